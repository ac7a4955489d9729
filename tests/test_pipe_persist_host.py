"""CPU tier: what the boxes of a pipe (include/mtgpu_pipe_boxes.h) and persistence on the decode path promise without a
device — the ABI, the header, the refusals that come before any HIP call, the host layer's surface — and the inputs of
tests/test_gpu_pipe_persist.py: the worked numbers against the models alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import blobs_model as bm
import persist_inputs as pi
import persist_model as pmod
import pipe_persist_inputs as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
NAMES = ["mtgpu_batch_boxes"]


# ------------------------------------------------------------------ the ABI and the sources

def test_layout_flag_is_exported_and_disjoint():
    assert m.LAYOUT_BOXES == _abi.LAYOUT_BOXES == 8 and "LAYOUT_BOXES" in m.__all__
    others = (m.LAYOUT_AOS40, m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES)
    assert all(m.LAYOUT_BOXES & o == 0 for o in others) and m.LAYOUT_COMPACT8 == 0
    hdr = open(os.path.join(ROOT, "include", "mtgpu_pipe_boxes.h")).read()
    assert re.search(r"^#define MT_LAYOUT_BOXES 8$", hdr, flags=re.M)


def test_abi_declares_what_the_header_declares():
    text = open(os.path.join(ROOT, "include", "mtgpu_pipe_boxes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", text))) == sorted(_abi.ABI_PIPE_BOXES) == NAMES
    lib = m.load_library()
    for n in NAMES:
        assert hasattr(lib, n)
    assert '#include "mtgpu_pipe_boxes.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\bT %s$" % n, exported, flags=re.M), n


def test_null_arguments_are_refused_without_a_device():
    lib = m.load_library()
    out = C.c_void_p(7)
    assert lib.mtgpu_batch_boxes(None, C.byref(out)) == _abi.MT_ERR_INVALID and out.value is None
    assert b"NULL" in lib.mtgpu_last_error()
    fake = C.create_string_buffer(64)                       # never dereferenced: the NULL result pointer is what is wrong
    assert lib.mtgpu_batch_boxes(fake, None) == _abi.MT_ERR_INVALID and b"NULL" in lib.mtgpu_last_error()
    assert lib.mtgpu_batch_boxes(None, None) == _abi.MT_ERR_INVALID
    # a NULL context is refused before the layout is looked at, whatever the layout
    pipe = C.c_void_p()
    for layout in (8, 15, 16):
        assert lib.mtgpu_pipe_create_layout(None, 100, 4, 2, layout, C.byref(pipe)) == _abi.MT_ERR_INVALID and not pipe.value


def test_header_compiles_alone_as_c_and_cpp(tmp_path):
    body = ("int use(const mtgpu_batch *b) {\n  const struct mt_blob_box *box = 0;\n"
            "  return mtgpu_batch_boxes(b, &box) + MT_LAYOUT_BOXES + (MT_LAYOUT_AOS40 | MT_LAYOUT_ZERO_COPY | MT_LAYOUT_CENTRES | MT_LAYOUT_BOXES)\n"
            "         + (box ? (int)box[0].x0 : 0);\n}\n")
    for first in ("mtgpu_pipe_boxes.h", "mtgpu.h", "mtgpu_persist.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_boxes.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])
    for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
        subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang, os.path.join(ROOT, "include", "mtgpu_pipe_boxes.h")])


def test_boxed_forms_of_both_kernels_are_in_the_library():
    """REC | kRecBoxed (0x100) selects them: 264 = 8 | 256, 296 = 40 | 256; the four forms each kernel had keep their names."""
    blob = open(_abi.LIB_PATH, "rb").read()
    for kern in (b"blobs_frames_kernel", b"gmc_blobs_frames_kernel"):
        for rec in (264, 296):
            assert kern + b"ILi1024ELi4ELi%dELb1EE" % rec in blob, (kern, rec)
        for rec in (8, 40):
            for pipe in (0, 1):
                assert kern + b"ILi1024ELi4ELi%dELb%dEE" % (rec, pipe) in blob, (kern, rec, pipe)


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.drain_boxes)
    import inspect
    assert "boxes" in inspect.signature(m.ScanPipe.__init__).parameters
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_persist(int min_run, uint32_t max_dropout = 0, int reach = -1)", "const std::vector<TraceEntry> &last_trace() const",
                 "struct TraceEntry {", "int min_run = -1;", "std::vector<int> run_sweep_levels;", "std::vector<SweepEntry> run_sweep;",
                 "size_t frames_before_persist = 0;", "inline PersistOptions &persist_options()", "MT_LAYOUT_BOXES"):
        assert text in host, text
    # ONE persistence call per recording, behind the pooling
    body = host[host.index("int run_scan_pipeline("):host.index("// ---------------------------------------------------------------- batch of videos")]
    assert body.count("mtgpu_persist_flags(") == 1 and body.index("for (auto &w : workers) w.join();") < body.index("mtgpu_persist_flags(")
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    for opt in ('"--min-run"', '"--max-dropout"', '"--reach"', '"--sweep-min-run"'):
        assert opt in tool
    for name in ("mtgpu_persist.h", "mtgpu_pipe_blobs.h", "mtgpu_pipe_gmc_blobs.h"):
        assert "mtgpu_pipe_boxes.h" in open(os.path.join(ROOT, "include", name)).read(), name


def test_plain_c_example_and_the_host_program_compile():
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_boxes_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_persist_two_videos.cpp")])


# ------------------------------------------------------------------ mtgpu_scan_file: usage errors before any device call

PER_LEVEL = ": a level sweep under persistence needs one persistence pass per level, which is not built"
NEEDS_BLOBS = "--reach needs --min-blob-cells N > 0 or --gmc-blobs N > 0: only a blob scan reports the box that --reach compares"
ONLY = " is valid only next to --min-run N > 1 or --sweep-min-run"


@pytest.mark.parametrize("args, text", [
    (["--min-run", "3", "--sweep", "2,3"], "--min-run cannot be combined with --sweep" + PER_LEVEL),
    (["--sweep-blobs", "4", "--min-run", "2"], "--min-run cannot be combined with --sweep-blobs" + PER_LEVEL),
    (["--min-run", "3", "--sweep-gmc-blobs", "3"], "--min-run cannot be combined with --sweep-gmc-blobs" + PER_LEVEL),
    (["--sweep-min-run", "1,3", "--sweep", "2"], "--sweep-min-run cannot be combined with --sweep" + PER_LEVEL),
    (["--sweep-min-run", "2", "--sweep-blobs", "4"], "--sweep-min-run cannot be combined with --sweep-blobs" + PER_LEVEL),
    (["--sweep-gmc-blobs", "3", "--sweep-min-run", "2"], "--sweep-min-run cannot be combined with --sweep-gmc-blobs" + PER_LEVEL),
    (["--min-run", "3", "--reach", "1"], NEEDS_BLOBS),
    (["--sweep-min-run", "2", "--reach", "0"], NEEDS_BLOBS),
    (["--min-run", "3", "--reach", "1", "--min-blob-cells", "0"], NEEDS_BLOBS),
    (["--min-run", "3", "--reach", "1", "--gmc"], NEEDS_BLOBS),
    (["--reach", "1", "--min-blob-cells", "3"], "--reach" + ONLY),
    (["--max-dropout", "2"], "--max-dropout" + ONLY),
    (["--min-run", "1", "--max-dropout", "2"], "--max-dropout" + ONLY),
    (["--min-run"], "--min-run takes an integer in [0, 2147483647]"),
    (["--min-run", "-1"], "--min-run takes an integer in [0, 2147483647]"),
    (["--min-run", "3x"], "--min-run takes an integer in [0, 2147483647]"),
    (["--min-run", "3", "--max-dropout", "4294967296"], "--max-dropout takes an integer in [0, 4294967295]"),
    (["--min-run", "3", "--reach", "65536", "--min-blob-cells", "1"], "--reach takes an integer in [0, 65535]"),
    (["--sweep-min-run"], "--sweep-min-run takes a comma-separated list of integers"),
    (["--sweep-min-run", "1,"], "--sweep-min-run takes a comma-separated list of integers"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_options_before_any_device_call(args, text):
    """Status 2, the stated text — both sides named — and an empty stdout.  The input does not exist and --streams 0 would
    ask for the device count: the refusal comes before either is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    env = {k: v for k, v in os.environ.items() if k != "CLUSTERS_NEEDED"}
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "", out.stderr


@pytest.mark.parametrize("args", [["--min-run", "3"], ["--min-run", "3", "--max-dropout", "4294967295"], ["--min-run", "3", "--centres"],
                                  ["--min-run", "3", "--reach", "2", "--min-blob-cells", "4"], ["--min-run", "3", "--reach", "0", "--gmc-blobs", "3"],
                                  ["--min-run", "2", "--gmc"], ["--sweep-min-run", "1,2,3,5", "--min-blob-cells", "2"],
                                  ["--min-run", "1", "--sweep", "2,3"], ["--min-run", "0", "--sweep-blobs", "4"]],
                         ids=lambda v: " ".join(v))
def test_what_combines_is_no_usage_error(args):
    """The tool goes on to look for its input."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--threads", "1", "--streams", "1"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 2 and "cannot be combined" not in out.stderr and "valid only" not in out.stderr and "needs" not in out.stderr


def test_the_pipeline_refuses_the_same_combinations_and_names_both_sides():
    """The whole sentences, as run_scan_pipeline and initialize() gave them on a GPU at the commit before the refusals became
    tables (tests/golden/host_mode_matrix.json); tests/test_scan_request_host.py holds csrc/host/scan_request.hpp to every
    recorded case."""
    import host_mode_matrix as hm
    _, scanner, pipeline = hm.load()
    said = {v[2] for v in pipeline.values()}
    for mine in ("min_run", "run_sweep_levels"):
        for other in ("sweep_levels", "blob_sweep_levels", "gmc_blob_sweep_levels"):
            assert mine + " together with " + other + ": a level sweep under persistence needs one persistence pass per level, which is " \
                "not built" in said, (mine, other)
    assert "reach without min_blob_cells / gmc_blob_cells: only a blob scan reports the box that reach compares" in said
    assert "set_persist with reach >= 0 needs set_min_blob_cells(n > 0) or set_gmc_blobs(n > 0): only a blob scan reports the box " \
        "that reach compares" in {v[0] for v in scanner.values()}


# ------------------------------------------------------------------ the worked numbers, by the models alone

def test_box_inputs_by_the_model():
    frames = pp.all_frames()
    assert len(frames) == 23 and len(frames) > 2 * pp.MAX_FRAMES             # at least three batches of five
    w = pp.expected("cn1", False)
    assert w["box"][17] == (60, 40, 63, 40)          # two blobs of 4 across the word seam: the upper-left one
    assert w["box"][20] == (20, 10, 22, 11) and w["box"][21] == (80, 10, 82, 11)      # the ties: the smallest y * gw + x wins
    assert w["box"][22] == (50, 0, 51, 67) and w["largest"][22] == 2 * 68
    assert pp.expected("margin3", False)["box"][22] == (50, 3, 51, 64)       # offset by the band's first row
    assert w["box"][0] == w["box"][4] == w["box"][5] == pp.NO_BOX              # no side data, no record, no centre
    for name in pp.settings():
        for masked in (False, True):
            e = pp.expected(name, masked)
            assert sum(e["flags"]) >= 5 and 0 in e["flags"]
            assert all((b == pp.NO_BOX) == (not fl) for b, fl in zip(e["box"], e["flags"]))
    # under the mask (columns 42 and 82 cleared) the block of 2 x 4 at columns 40 .. 43 keeps columns 40 .. 41
    assert pp.expected("cn1", True)["box"][18] == (40, 30, 41, 31) and w["box"][18] == (40, 30, 43, 31)
    p, mb, one, two, b1, f2, b2 = pp.stale_case()
    for batch, boxes in ((one, b1), (two, b2)):
        mv, off, sd = pp.pb.batch_arrays(batch)
        st = bm.model_batch(p, mv, off, sd)
        fl = bm.flags_np(p, st["centres"], st["largest"], mb).tolist()
        assert [tuple(b) if f else pp.NO_BOX for b, f in zip(st["box"].tolist(), fl)] == boxes
        assert fl == ([1, 1, 1, 1] if batch is one else f2)


def test_seam_recording_by_the_model():
    """M frames 8 9 10 | 19 (key frame 20) 21 22 | 33: MIN_RUN 3 keeps the first six."""
    kept, runs = pp.seam_expected(3, 0)
    assert tuple(kept) == pp.SEAM_KEPT == (8, 9, 10, 19, 21, 22) and runs[33] == 1 and runs[20] == 0
    # what a rule applied per one-second chunk would keep: nothing but ... nothing — every chunk holds at most two M frames of a run
    fl, sd = pp.seam_classes()
    per_chunk = []
    for a in range(0, 40, 10):
        r = pmod.persist(fl[a:a + 10], [0, 10], has_sd=sd[a:a + 10], min_run=3)
        per_chunk += [a + f for f in range(10) if r["flags"][f]]
    assert per_chunk == []
    assert pp.seam_expected(2, 0, (9,))[0] == [19, 21, 22] and pp.seam_expected(2, 1, (9,))[0] == [8, 10, 19, 21, 22]
    fr = pp.seam_frames()
    assert [f is None for f in fr] == [i in pp.SEAM_KEYS for i in range(40)]
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1)
    mv, off, sdv = pp.pb.batch_arrays(fr)
    st = bm.model_batch(p, mv, off, sdv)
    assert bm.flags_np(p, st["centres"], st["largest"], 1).tolist() == fl.tolist()


def test_end_to_end_numbers_by_the_models():
    """29 frames with boxes at reach 1, 30 without, 33 before persistence; the run sweep's 33 / 29 / 29 / 29."""
    p, mv, off, sd = pi.e2e_stream()
    st = bm.model_batch(p, mv, off, sd)
    flags = bm.flags_np(p, st["centres"], st["largest"], 1)
    n = len(flags)
    assert int(flags.sum()) == 33
    boxed = pmod.persist(flags, [0, n], sd, st["box"], min_run=3, max_dropout=0, reach=1)
    assert np.flatnonzero(boxed["flags"]).tolist() == pi.E2E_KEPT == list(range(121, 150))
    loose = pmod.persist(flags, [0, n], sd, None, min_run=3)
    assert np.flatnonzero(loose["flags"]).tolist() == [119] + pi.E2E_KEPT
    assert [int((boxed["run"] >= L).sum()) for L in (1, 2, 3, 5)] == [33, 29, 29, 29]
    assert 135 in pi.E2E_KEPT and abs((3000 * 135) * (1.0 / 90000.0) - 4.5) < 1e-12      # the chunk border inside the event


def test_example_numbers_by_the_models():
    loose, boxed = pp.example_expected()
    assert len(loose) == 145 and len(boxed) == 58 and boxed == [f for f in range(200, 260) if f % 30]
    assert loose == [f for f in list(range(60, 150)) + list(range(200, 260)) if f % 30]
