"""CPU tier: what the compensated blob scan through the pipe (include/mtgpu_pipe_gmc_blobs.h) promises without a device —
the ABI, the headers, the refusals that come before any HIP call, the texts with which the two single modes still refuse
each other — and the inputs of tests/test_gpu_pipe_gmc_blobs.py: the hand values against the model."""
import ctypes as C
import os
import re
import subprocess

import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import gmc_blobs_inputs as gbi
import pipe_blobs_inputs as pbi
import pipe_gmc_blobs_inputs as pq
import pipe_gmc_inputs as pgi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
NAMES = ["mtgpu_pipe_gmc_blobs", "mtgpu_pipe_set_gmc_blobs"]


# ------------------------------------------------------------------ the ABI and the sources

def test_abi_declares_what_the_header_declares():
    text = open(os.path.join(ROOT, "include", "mtgpu_pipe_gmc_blobs.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", text))) == sorted(_abi.ABI_PIPE_GMC_BLOBS) == NAMES
    lib = m.load_library()
    for n in NAMES:
        assert hasattr(lib, n)
    assert '#include "mtgpu_pipe_gmc_blobs.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert (_abi.MT_PIPE_REPORT_CENTRES, _abi.MT_PIPE_REPORT_LARGEST, _abi.MT_PIPE_REPORT_VECTOR) == (0, 1, 2)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\bT %s$" % n, exported, flags=re.M), n


def test_null_pipe_is_refused_without_a_device():
    lib = m.load_library()
    assert lib.mtgpu_pipe_set_gmc_blobs(None, 3, 16, 128, 0) == _abi.MT_ERR_INVALID and b"pipe is NULL" in lib.mtgpu_last_error()
    assert lib.mtgpu_pipe_set_gmc_blobs(None, 0, 0, 0, 0) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_pipe_gmc_blobs(None, None, None, None, None) == -1
    a = C.c_int32(7)
    assert lib.mtgpu_pipe_gmc_blobs(None, C.byref(a), None, None, None) == -1 and a.value == 7


def test_all_four_forms_of_the_kernel_are_in_the_library_and_the_submit_tests_the_pair_first():
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        for pipe in (0, 1):
            assert b"gmc_blobs_frames_kernelILi1024ELi4ELi%dELb%dEE" % (rec, pipe) in blob, (rec, pipe)
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    assert pipe_src.count("getenv") == 4
    assert "getenv" not in open(os.path.join(PKG, "csrc", "gmc_blobs_kernels.hip")).read()
    # which scan a submit runs is the pipe's ONE mode (csrc/pipe_mode.h), so there is no order of tests left to hold: that no
    # second mode can be on next to this one is held by cases (a) and (b) of tests/golden/pipe_mode_matrix.json, recorded from
    # the commit before the modes became one value, together with this mode's result tests (tests/test_gpu_pipe_gmc_blobs.py)
    import pipe_mode_matrix as pm
    assert pm.excludes_every_other("gmc_blobs")


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_pipe *p) {\n  int32_t a = 0, b = 0, c = 0;\n  int r = 0;\n"
            "  return mtgpu_pipe_set_gmc_blobs(p, 3, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_VECTOR)\n"
            "       + mtgpu_pipe_set_gmc_blobs(p, 0, 0, 0, MT_PIPE_REPORT_LARGEST) + mtgpu_pipe_gmc_blobs(p, &a, &b, &c, &r)\n"
            "       + mtgpu_pipe_gmc_blobs(p, 0, 0, 0, 0) + (int)a + (int)b + (int)c + r + MT_PIPE_REPORT_CENTRES;\n}\n")
    for first in ("mtgpu.h", "mtgpu_pipe_gmc_blobs.h", "mtgpu_gmc_blobs.h", "mtgpu_pipe_gmc.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_gmc_blobs.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_gmc_blobs) and callable(m.ScanPipe.clear_gmc_blobs) and callable(m.ScanPipe.gmc_blobs)
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_gmc_blobs(int min_blob_cells, int max_shift = MTGPU_GMC_DEFAULT_MAX_SHIFT, int min_share_q8 = MTGPU_GMC_DEFAULT_MIN_SHARE_Q8)",
                 "void report_gmc_blobs(int report)", "int gmc_blob_cells = -1;", "int gmc_blob_max_shift", "int gmc_blob_min_share_q8",
                 "std::vector<int> gmc_blob_sweep_levels;", "std::vector<SweepEntry> gmc_blob_sweep;",
                 "inline GmcBlobOptions &gmc_blob_options()"):
        assert text in host, text
    # initialize() turns every mode off before it settles this video's one (all_off): held on a GPU by the 36 "the previous
    # video ran X, this video asks Y" pairs of tests/test_gpu_host_mode_matrix.py
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    for opt in ('"--gmc-blobs"', '"--gmc-blobs-max-shift"', '"--gmc-blobs-min-share-q8"', '"--sweep-gmc-blobs"'):
        assert opt in tool


def test_plain_c_example_and_the_host_program_compile():
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_gmc_blobs_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_gmc_blobs_two_videos.cpp")])


# ------------------------------------------------------------------ mtgpu_scan_file: usage errors before any device call

OWN_GMC = "the compensated blob scan has its own compensation"
OWN_SIZE = "the compensated blob scan has its own minimum blob size"
ONLY = " is valid only next to --gmc-blobs or --sweep-gmc-blobs"
ONE_ARRAY = "--sweep-gmc-blobs cannot be combined with --centres or --sweep: a pipe has one count array"


@pytest.mark.parametrize("args, text", [
    (["--gmc-blobs", "3", "--gmc"], "--gmc-blobs cannot be combined with --gmc: " + OWN_GMC),
    (["--gmc-max-shift", "4", "--gmc-blobs", "3"], "--gmc-blobs cannot be combined with --gmc-max-shift: " + OWN_GMC),
    (["--gmc-blobs", "3", "--gmc-min-share-q8", "64"], "--gmc-blobs cannot be combined with --gmc-min-share-q8: " + OWN_GMC),
    (["--gmc-vectors", "--gmc-blobs", "3"], "--gmc-blobs cannot be combined with --gmc-vectors: " + OWN_GMC),
    (["--sweep-gmc-blobs", "3,8", "--gmc"], "--sweep-gmc-blobs cannot be combined with --gmc: " + OWN_GMC),
    (["--gmc-blobs", "3", "--min-blob-cells", "3"], "--gmc-blobs cannot be combined with --min-blob-cells: " + OWN_SIZE),
    (["--sweep-blobs", "4", "--gmc-blobs", "3"], "--gmc-blobs cannot be combined with --sweep-blobs: " + OWN_SIZE),
    (["--sweep-gmc-blobs", "3", "--min-blob-cells", "2"], "--sweep-gmc-blobs cannot be combined with --min-blob-cells: " + OWN_SIZE),
    (["--sweep-gmc-blobs", "3", "--sweep-blobs", "4"], "--sweep-gmc-blobs cannot be combined with --sweep-blobs: " + OWN_SIZE),
    (["--sweep-gmc-blobs", "3,8", "--centres"], ONE_ARRAY),
    (["--sweep", "2,3", "--sweep-gmc-blobs", "3"], ONE_ARRAY),
    (["--gmc-blobs-max-shift", "4"], "--gmc-blobs-max-shift" + ONLY),
    (["--gmc-blobs-min-share-q8", "64"], "--gmc-blobs-min-share-q8" + ONLY),
    (["--gmc-blobs", "0", "--gmc-blobs-max-shift", "4"], "--gmc-blobs-max-shift" + ONLY),
    (["--gmc", "--gmc-blobs-min-share-q8", "64"], "--gmc-blobs-min-share-q8" + ONLY),
    (["--gmc-blobs", "3", "--gmc-blobs-max-shift", "128"], "--gmc-blobs-max-shift takes an integer in [0, 127]"),
    (["--gmc-blobs", "3", "--gmc-blobs-max-shift"], "--gmc-blobs-max-shift takes an integer in [0, 127]"),
    (["--gmc-blobs", "3", "--gmc-blobs-min-share-q8", "257"], "--gmc-blobs-min-share-q8 takes an integer in [0, 256]"),
    (["--gmc-blobs", "-1"], "--gmc-blobs takes a cell count >= 0"),
    (["--gmc-blobs", "3x"], "--gmc-blobs takes a cell count >= 0"),
    (["--gmc-blobs"], "--gmc-blobs takes a cell count >= 0"),
    (["--sweep-gmc-blobs"], "--sweep-gmc-blobs takes a comma-separated list of integers"),
    (["--sweep-gmc-blobs", "3,"], "--sweep-gmc-blobs takes a comma-separated list of integers"),
    (["--sweep-gmc-blobs", "1,3"], "--sweep-gmc-blobs level 1 is below max(1, CLUSTERS_NEEDED) = 2"),
    # the refusals the two single modes had before: word for word
    (["--gmc", "--min-blob-cells", "3"], "--gmc cannot be combined with --min-blob-cells or --sweep-blobs: compensation and blobs are not together yet"),
    (["--sweep-blobs", "4", "--gmc-max-shift", "5"], "--gmc cannot be combined with --min-blob-cells or --sweep-blobs: compensation and blobs are not together yet"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_options_before_any_device_call(args, text):
    """Status 2, the stated text and an empty stdout.  The input does not exist and --streams 0 would ask for the device
    count: the refusal comes before either is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    env = {k: v for k, v in os.environ.items() if k != "CLUSTERS_NEEDED"}
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "", out.stderr


@pytest.mark.parametrize("args", [["--gmc-blobs", "3", "--centres"], ["--gmc-blobs", "3", "--sweep", "2,3"],
                                  ["--gmc-blobs", "0", "--gmc"], ["--gmc-blobs", "3", "--min-blob-cells", "0"],
                                  ["--gmc-blobs", "3", "--gmc-blobs-max-shift", "0", "--gmc-blobs-min-share-q8", "256"]],
                         ids=lambda v: " ".join(v))
def test_what_combines_is_no_usage_error(args):
    """The tool goes on to look for its input."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--threads", "1", "--streams", "1"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 2 and "cannot be combined" not in out.stderr and "valid only" not in out.stderr


def test_the_single_modes_still_refuse_each_other_in_the_same_words():
    """The whole sentences, as a GPU answered them at the commit before the refusals became tables (tests/golden/
    pipe_mode_matrix.json, host_mode_matrix.json); tests/test_pipe_mode_host.py and tests/test_scan_request_host.py hold the
    tables to every one of them."""
    import host_mode_matrix as hm
    import pipe_mode_matrix as pm
    ans = pm.recorded()
    assert (ans["a/gmc/blobs"][1]["rc"], ans["a/gmc/blobs"][1]["error"]) == \
        (_abi.MT_ERR_UNSUPPORTED, "this pipe runs the compensated scan (mtgpu_pipe_set_gmc): blobs and compensation are not together yet")
    assert (ans["a/blobs/gmc"][1]["rc"], ans["a/blobs/gmc"][1]["error"]) == \
        (_abi.MT_ERR_UNSUPPORTED, "this pipe runs the blob scan (mtgpu_pipe_set_blobs): blobs and compensation are not together yet")
    _, scanner, pipeline = hm.load()
    assert "compensation and blobs are not together yet" in {v[0] for v in scanner.values()}
    assert "compensation together with min_blob_cells / blob_sweep_levels: not together yet" in {v[2] for v in pipeline.values()}
    for name in ("mtgpu_gmc_blobs.h", "mtgpu_pipe_gmc.h", "mtgpu_pipe_blobs.h"):
        assert "mtgpu_pipe_gmc_blobs.h" in open(os.path.join(ROOT, "include", name)).read(), name
    assert "mtgpu_pipe_gmc_blobs.h" in open(os.path.join(PKG, "csrc", "gmc_blobs_kernels.hip")).read()


# ------------------------------------------------------------------ the inputs, by the model

def test_hand_values_of_the_rule_by_the_model():
    p = pgi.params()
    fr = gbi.bite_frames()
    assert p.clusters_needed == 2 and pq.MIN_BLOB == 3 and (pq.MS, pq.Q8) == (16, 128)
    spelled = {"P4": (0, 8, 2), "O8": (1, 8, 8), "P4+overlay, no mask": (1, 38, 30), "P4+overlay, mask": (0, 8, 2)}
    for row in pq.BITE:
        name, frame, kp, flag, centres, largest, vec = row
        assert (flag, centres, largest) == spelled[name] and vec == (9, 3)
        assert fr[frame].dtype.itemsize == 40
        keep = gbi.BITE_KEEPS[kp]
        for report in pq.REPORTS:
            assert pq.model(p, [fr[frame]], pq.MIN_BLOB, pq.MS, pq.Q8, report, keep) == ([flag], [pq.bite_count(row, report)]), (name, report)
    # the hand table of gmc_blobs_inputs says the same
    for (name, frame, kp, stats, info), row in zip(gbi.BITE_HAND, pq.BITE):
        assert (name, frame, kp) == row[:3] and (stats[0], stats[2]) == row[4:6] and tuple(info[:2]) == row[6]
    # the single modes on P4 and O8: set_gmc flags both (8 centres), set_blobs(3) flags both (one blob of 2360)
    for f in ("P4", "O8"):
        fl, ce, _ = pgi.model(p, [fr[f]], pq.MS, pq.Q8)
        assert (fl[0], ce[0]) == pq.BITE_GMC_ALONE
        mo = pbi.model(p, [fr[f]])
        assert (pbi.flags_of(p, mo, 3)[0], mo["centres"][0], mo["largest"][0]) == pq.BITE_BLOBS_ALONE
    # under the mask applied only to the active plane case D keeps its 40 centres; with the masked estimate it has none
    d = fr["D"]
    assert pq.model(p, [d], 3, pq.MS, pq.Q8, "centres", pgi.KEEP_D) == ([0], [0])
    assert pq.model(p, [d], 3, pq.MS, pq.Q8, "vector", pgi.KEEP_D) == ([0], [pgi.pack_vector(9, 3)])
    assert pq.model(p, [d], 3, pq.MS, pq.Q8, "centres") == ([1], [40])


def test_answer_and_q5():
    p = pgi.params()
    assert pq.answer(p, (8, 4, 2, None), (9, 3), 3, "centres") == (0, 8)
    assert pq.answer(p, (8, 4, 2, None), (9, 3), 2, "largest") == (1, 2)
    assert pq.answer(p, (1, 1, 1, None), (-9, -3), 1, "vector") == (0, pgi.pack_vector(-9, -3))      # one centre < CLUSTERS_NEEDED 2
    assert pq.answer(p, (8, 1, 8, None), (0, 0), 8, "vector") == (1, 0)
    for report in pq.REPORTS:
        assert pq.model(p, [None, None], 1, 16, 128, report) == ([0, 0], [0, 0])


def test_stale_case_by_the_model():
    p, one, two, three, hand = pq.stale_case()
    for frames, h in zip((one, two, three), hand):
        for report in pq.REPORTS:
            assert pq.model(p, frames, pq.MIN_BLOB, pq.MS, pq.Q8, report) == (h["flags"], h[report]), report
    assert hand[0]["vector"] != hand[1]["vector"] != hand[2]["vector"]


def test_seam_and_vn0_cases_by_the_model():
    p, plain, masked, keep, hand = pq.seam_case()
    assert all(f.dtype == m.MV_DTYPE and f.dtype.itemsize == 40 for f in plain + masked)
    # consequence C: under the embedding the unmasked frames read the hand values of pipe_blobs_inputs.seam_case
    assert pq.model(p, plain, 1, pq.MS, pq.Q8, "centres")[1] == hand["centres"]
    assert pq.model(p, plain, 1, pq.MS, pq.Q8, "largest")[1] == hand["largest"]
    assert pq.model(p, plain, 1, pq.MS, pq.Q8, "vector")[1] == [pgi.pack_vector(*pq.SEAM_PAN)] * len(plain)
    # column 63 cleared: frame 0's run of 8 falls into 3 + 4, frame 3's 4 + 4 into 3 + 4
    got = pq.model(p, masked, 1, pq.MS, pq.Q8, "largest", keep)[1]
    assert got[0] == 4 and got[3] == 4 and got != hand["largest"]
    p0, frames, keep0 = pq.vn0_case()
    c = pq.model(p0, frames, 1, pq.MS, pq.Q8, "centres", keep0)[1][0]
    g = pq.model(p0, frames, 1, pq.MS, pq.Q8, "largest", keep0)[1][0]
    assert 0 < g < c < 118 * 68


def test_batch_answers_equal_the_frame_model():
    p, frames, keep, has, plain, masked = pq.random_case(1)
    for report in pq.REPORTS:
        assert pq.batch_answers(p, plain, has, 2, report) == pq.model(p, frames, 2, pq.MS, 64, report)
        assert pq.batch_answers(p, masked, has, 2, report) == pq.model(p, frames, 2, pq.MS, 64, report, keep)
    assert not all(has) and [f is None for f in frames] == [not h for h in has]
