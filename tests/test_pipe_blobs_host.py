"""CPU tier: the blob setting of a pipe (include/mtgpu_pipe_blobs.h) exists at every layer — header, library, ctypes
table, ScanPipe, the C++ host layer, mtgpu_scan_file — and answers bad calls before any HIP call; and the inputs of
tests/test_gpu_pipe_blobs.py give, by the flood-fill model (tests/blobs_model.py), every number derived by hand in
tests/pipe_blobs_inputs.py: the GPU tier rests on values proven without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import pipe_blobs_inputs as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
NEW_SYMBOLS = ["mtgpu_pipe_blobs", "mtgpu_pipe_set_blobs"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_pipe_blobs.h")).read()


# ------------------------------------------------------------------ exports and early errors

def test_entry_points_are_declared_exported_and_refuse_a_null_pipe():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_PIPE_BLOBS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_PIPE_BLOBS[n][1], n
        assert n not in _abi.ABI
        # every declaration cites the reference lines it stands for: the centre test and the check_frame call site
        at = hdr.index("int " + n + "(")
        comment = hdr[hdr.rindex("\n/*", 0, at):at]
        assert "src/motion_scanner.cpp:272-294" in comment and ":375-383" in comment, n
    assert '#include "mtgpu_pipe_blobs.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert re.search(r"#define MT_PIPE_REPORT_CENTRES 0\b", hdr) and re.search(r"#define MT_PIPE_REPORT_LARGEST 1\b", hdr)
    assert (_abi.MT_PIPE_REPORT_CENTRES, _abi.MT_PIPE_REPORT_LARGEST) == (0, 1)
    # the contract lines the GPU tests rest on
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("centres >= max(1, clusters_needed) AND largest >= min_blob_cells", "MT_ERR_BUSY", "commute",
                 "A frame without side data reads flag 0 and count 0 under either report", "no `blobs` and no `box` through the pipe",
                 "give the segments of min_blob_cells = L, bit for bit", "records one event triple"):
        assert text in flat, text
    # a NULL pipe: answered from the arguments alone, no device needed
    assert lib.mtgpu_pipe_set_blobs(None, 3, 0) == _abi.MT_ERR_INVALID
    assert "NULL" in lib.mtgpu_last_error().decode()
    assert lib.mtgpu_pipe_set_blobs(None, 0, 0) == _abi.MT_ERR_INVALID
    n, r = C.c_int32(7), C.c_int(7)
    assert lib.mtgpu_pipe_blobs(None, C.byref(n), C.byref(r)) == -1 and (n.value, r.value) == (7, 7)
    assert lib.mtgpu_pipe_blobs(None, None, None) == -1
    # no new layout bit, no new environment variable
    assert (m.LAYOUT_AOS40 | m.LAYOUT_ZERO_COPY | m.LAYOUT_CENTRES) == 7
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    parent_env = {"MTGPU_INJECT_SUBMIT_FAIL", "MTGPU_INJECT_GROW_FAIL", "MTGPU_INJECT_COLLECT_FAIL", "MTGPU_INJECT_ONCE"}
    assert set(re.findall(r'getenv\("([A-Z_]+)"\)', pipe_src)) == parent_env and pipe_src.count("getenv") == 4
    assert "getenv" not in open(os.path.join(PKG, "csrc", "blobs_kernels.hip")).read()
    # both forms of the kernel are in the library, for both record layouts
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        for pipe in (0, 1):
            assert b"blobs_frames_kernelILi1024ELi4ELi%dELb%dEE" % (rec, pipe) in blob, (rec, pipe)


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_pipe *p) {\n  int32_t n = 0;\n  int r = 0;\n"
            "  return mtgpu_pipe_set_blobs(p, 3, MT_PIPE_REPORT_LARGEST) + mtgpu_pipe_set_blobs(p, 0, MT_PIPE_REPORT_CENTRES)\n"
            "       + mtgpu_pipe_blobs(p, &n, &r) + mtgpu_pipe_blobs(p, 0, 0) + (int)n + r;\n}\n")
    for first in ("mtgpu.h", "mtgpu_pipe_blobs.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_blobs.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_blobs) and isinstance(m.ScanPipe.blobs, property)
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_min_blob_cells(int n)", "void report_largest(bool on)", "int min_blob_cells = -1;",
                 "std::vector<int> blob_sweep_levels;", "inline BlobOptions &blob_options()",
                 "scanners[i]->set_min_blob_cells(out.min_blob_cells)"):
        assert text in host, text
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    assert '"--min-blob-cells"' in tool and '"--sweep-blobs"' in tool


def test_plain_c_example_and_the_host_program_compile(tmp_path):
    """examples/pipe_blobs_example.c and tests/cpp/pipe_blobs_two_videos.cpp against the headers as they are (they run
    in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_blobs_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_blobs_two_videos.cpp")])


@pytest.mark.parametrize("args, text", [
    (["--sweep-blobs", "8", "--centres"], "--sweep-blobs cannot be combined with --centres or --sweep"),
    (["--centres", "--sweep-blobs", "8"], "--sweep-blobs cannot be combined with --centres or --sweep"),
    (["--sweep-blobs", "8", "--sweep", "1,2"], "--sweep-blobs cannot be combined with --centres or --sweep"),
    (["--sweep-blobs", "2,1"], "--sweep-blobs level 1 is below max(1, CLUSTERS_NEEDED) = 2"),
    (["--sweep-blobs", "0"], "--sweep-blobs level 0 is below max(1, CLUSTERS_NEEDED) = 2"),
    (["--sweep-blobs", "8,,9"], "--sweep-blobs takes a comma-separated list of integers"),
    (["--sweep-blobs", "8,"], "--sweep-blobs takes a comma-separated list of integers"),
    (["--sweep-blobs", "8,x"], "--sweep-blobs takes a comma-separated list of integers"),
    (["--sweep-blobs", ""], "--sweep-blobs takes a comma-separated list of integers"),
    (["--sweep-blobs"], "--sweep-blobs takes a comma-separated list of integers"),
    (["--min-blob-cells", "-1"], "--min-blob-cells takes a cell count >= 0"),
    (["--min-blob-cells", "3x"], "--min-blob-cells takes a cell count >= 0"),
    (["--min-blob-cells"], "--min-blob-cells takes a cell count >= 0"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_blob_options_before_any_device_call(args, text):
    """Status 2 and a message naming the option.  The input does not exist and --streams 0 would ask for the device
    count: the refusal comes before either is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    env = {k: v for k, v in os.environ.items() if k != "CLUSTERS_NEEDED"}
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "", out.stderr
    # the level bound follows CLUSTERS_NEEDED
    if "level" in text:
        out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0", "--sweep-blobs", "7,9"], capture_output=True, text=True,
                             timeout=60, env=dict(env, CLUSTERS_NEEDED="8"))
        assert out.returncode == 2 and "--sweep-blobs level 7 is below max(1, CLUSTERS_NEEDED) = 8" in out.stderr


# ------------------------------------------------------------------ the inputs of the GPU tier, by the model

def assert_model(p, frames, hand, keep=None):
    mo = pb.model(p, frames, keep)
    for k, v in hand.items():
        if k != "flags":
            assert mo[k] == list(v), (k, mo[k], v)
    return mo


def test_hand_values_of_the_rule_seam_mask_and_stale_cases():
    p, frames, hand = pb.bite_case()
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.clusters_needed, p.vectors_needed) == (120, 68, 0, 8, 1)
    mo = assert_model(p, frames, hand)
    assert pb.flags_of(p, mo, 0) == [1, 1] and pb.flags_of(p, mo, 3) == [0, 1]
    p, frames, hand = pb.seam_case()
    assert_model(p, frames, hand)
    p, frames, hand = pb.vn0_case()
    assert (p.vectors_needed, p.vertical_margin) == (0, 0)
    assert_model(p, frames, hand)
    p, frames, keep, plain, masked = pb.mask_case()
    mo = assert_model(p, frames, plain)
    assert pb.flags_of(p, mo, pb.MASK_MIN_BLOB) == [1, 1]
    mo = assert_model(p, frames, masked, keep)
    assert pb.flags_of(p, mo, pb.MASK_MIN_BLOB) == [0, 0] and pb.flags_of(p, mo, 1) == [0, 1]
    p, one, two, h1, h2 = pb.stale_case()
    assert pb.flags_of(p, assert_model(p, one, h1), pb.MIN_BLOB) == h1["flags"]
    mo = assert_model(p, two, h2)
    assert pb.flags_of(p, mo, pb.MIN_BLOB) == h2["flags"] and pb.flags_of(p, mo, 1) == [1, 0, 0]


def test_shape_4k_and_recording_inputs_do_what_the_gpu_cases_need():
    p, frames = pb.shapes_case()
    mo = pb.model(p, frames)
    fl = pb.flags_of(p, mo, pb.MIN_BLOB)
    assert frames[0] is None and frames[6] is None and frames[-1] is None and len(frames[4]) == 0
    assert len({len(f) for f in frames if f is not None}) >= 6                       # ragged
    assert 0 in fl and 1 in fl and fl != pb.flags_of(p, mo, 1)                       # the rule changes some frame's flag
    assert mo["centres"] != mo["largest"]                                             # the two reports differ
    assert mo["largest"][1] == 2 and mo["centres"][5] == 0 and mo["largest"][7] == 12
    assert mo["largest"][9] == 40 and mo["largest"][12] == 40                         # column 0 / column gw - 1 are no centres
    p, frames = pb.uhd_case()
    mo = pb.model(p, frames)
    assert mo["largest"] == [360, 2, 360, 0, 0, 476] and mo["centres"] == [360, 10, 370, 0, 0, 476] and mo["blobs"][1] == 5
    p, frames, pts, keep = pb.recording_case()
    assert pb.model(p, frames)["largest"] == pb.REC_LARGEST and pb.model(p, frames, keep)["largest"] == pb.REC_LARGEST_MASKED
    assert len(pts) == pb.REC_FRAMES and min(pb.model(p, frames, keep)["centres"]) >= p.clusters_needed
