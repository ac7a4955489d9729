"""CPU tier: what direction planes through the pipe (include/mtgpu_pipe_lanes.h) promise without a device — the ABI, the
header, the refusals that come before any HIP call, the host layer's plane loader — and the inputs and the model of
tests/test_gpu_pipe_lanes.py: every hand-derived number against the model, the model against the unchanged oracle through
removal on every input, and the preview facts the limit cases rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, lanes

import derived_cliff_inputs as dc
import dir_inputs as di
import lanes_inputs as li
import lanes_model as lm
import pipe_dir_inputs as pd
import pipe_lanes_inputs as pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)


# ------------------------------------------------------------------ the ABI and the sources

def test_abi_declares_what_the_header_declares_and_the_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "mtgpu_pipe_lanes.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", text))) == sorted(_abi.ABI_PIPE_LANES) == ["mtgpu_pipe_plane", "mtgpu_pipe_set_plane"]
    lib = m.load_library()
    for n in _abi.ABI_PIPE_LANES:
        assert hasattr(lib, n)
    assert '#include "mtgpu_pipe_lanes.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    for other in ("mtgpu_lanes.h", "mtgpu_pipe_dir.h"):                            # one pointer each, in the "Out of scope" sentence
        assert open(os.path.join(ROOT, "include", other)).read().count("mtgpu_pipe_lanes.h") == 1, other


def test_null_pipe_is_refused_without_a_device():
    lib = m.load_library()
    plane = np.zeros(30, dtype=np.uint8)
    assert lib.mtgpu_pipe_set_plane(None, plane.ctypes.data_as(C.c_void_p), 0) == _abi.MT_ERR_INVALID
    assert b"pipe is NULL" in lib.mtgpu_last_error()
    assert lib.mtgpu_pipe_set_plane(None, None, 0) == _abi.MT_ERR_INVALID
    r = C.c_int(7)
    assert lib.mtgpu_pipe_plane(None, None, C.byref(r)) == -1 and r.value == 7


def test_four_forms_of_the_kernel_are_in_the_library_and_the_pipe_reads_no_new_environment():
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        for staged in (0, 1):
            assert b"lanes_pipe_kernelILi1024ELi4ELi%dELb%dEE" % (rec, staged) in blob, (rec, staged)
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    assert pipe_src.count("getenv") == 4
    assert "getenv" not in open(os.path.join(PKG, "csrc", "lanes_kernels.hip")).read()
    # which scan a submit runs is the pipe's ONE mode (csrc/pipe_mode.h), so there is no order of tests left to hold: that no
    # second mode can be on next to this one is held by cases (a) and (b) of tests/golden/pipe_mode_matrix.json, recorded from
    # the commit before the modes became one value, together with this mode's result tests (tests/test_gpu_pipe_lanes.py)
    import pipe_mode_matrix as pm
    assert pm.excludes_every_other("plane")


def test_header_compiles_alone_as_c11_and_as_cpp17(tmp_path):
    body = ("int use(mtgpu_pipe *p, const uint8_t *plane, uint8_t *back) {\n  int r = 0;\n"
            "  return mtgpu_pipe_set_plane(p, plane, MT_PIPE_REPORT_SECTORS) + mtgpu_pipe_set_plane(p, 0, MT_PIPE_REPORT_CENTRES)\n"
            "       + mtgpu_pipe_plane(p, back, &r) + mtgpu_pipe_plane(p, 0, 0) + r;\n}\n")
    for first in ("mtgpu_pipe_lanes.h", "mtgpu.h", "mtgpu_lanes.h", "mtgpu_pipe_dir.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_lanes.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_plane) and callable(m.ScanPipe.clear_plane) and isinstance(m.ScanPipe.plane, property)
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_plane(const std::vector<uint8_t> &plane)", "inline bool load_plane(const std::string &path, int gw, int gh,",
                 "std::vector<uint8_t> dir_plane;", "inline PlaneOptions &plane_options()", "plane_for"):
        assert text in host, text
    # initialize() turns every mode off before it settles this video's one (all_off): held on a GPU by the 36 "the previous
    # video ran X, this video asks Y" pairs of tests/test_gpu_host_mode_matrix.py
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    assert '"--plane"' in tool


def test_plain_c_example_and_the_host_program_compile():
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_lanes_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_lanes_two_videos.cpp")])


def test_set_plane_checks_shape_dtype_and_report_before_any_call():
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    class Scanner:
        params = pd.small_params()
    pipe = m.ScanPipe.__new__(m.ScanPipe)
    pipe._lib, pipe._pipe, pipe._scanner = NoLibrary(), None, Scanner()
    good = np.zeros((5, 6), dtype=np.uint8)
    for report in ("vector", "largest", "rose", "", None, 3):
        with pytest.raises(ValueError):
            pipe.set_plane(good, report)
    for bad in (np.zeros((6, 5), np.uint8), np.zeros(30, np.uint8), np.zeros((5, 6), np.int32), np.zeros((5, 6), bool),
                np.zeros((1, 5, 6), np.uint8)):
        with pytest.raises(ValueError):
            pipe.set_plane(bad)
    pipe._pipe = None                                                          # (close() finds nothing to destroy)


# ------------------------------------------------------------------ mtgpu_host::load_plane

LOADER = r"""
#include <cstdio>
#include "mtgpu_host.hpp"
int main(int argc, char **argv) {
  if (argc != 4) return 3;
  std::vector<uint8_t> bytes;
  std::string err;
  if (!mtgpu_host::load_plane(argv[1], std::atoi(argv[2]), std::atoi(argv[3]), bytes, err)) {
    std::printf("error %s\n", err.c_str());
    return 1;
  }
  std::printf("ok");
  for (uint8_t b : bytes) std::printf(" %u", (unsigned)b);
  std::printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def loader(tmp_path_factory):
    d = tmp_path_factory.mktemp("plane_loader")
    src = d / "plane_loader.cpp"
    src.write_text(LOADER)
    exe = str(d / "plane_loader")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), str(src), "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, d


def run_loader(exe, path, gw, gh):
    out = subprocess.run([exe, str(path), str(gw), str(gh)], capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout.strip()


def test_load_plane_reads_what_save_plane_writes(loader):
    exe, d = loader
    rng = np.random.RandomState(77)
    for gw, gh in ((6, 5), (65, 9), (1, 1), (120, 68)):
        plane = rng.randint(0, 256, size=(gh, gw)).astype(np.uint8)
        path = d / f"p_{gw}x{gh}.mtdir"
        lanes.save_plane(str(path), plane)
        assert np.array_equal(lanes.load_plane(str(path), (gw, gh)), plane)
        rc, text = run_loader(exe, path, gw, gh)
        assert rc == 0 and text.split()[0] == "ok" and [int(x) for x in text.split()[1:]] == plane.ravel().tolist(), (gw, gh)
        crlf = d / f"p_{gw}x{gh}_crlf.mtdir"
        crlf.write_bytes(path.read_bytes().replace(b"\n", b"\r\n"))
        assert np.array_equal(lanes.load_plane(str(crlf), (gw, gh)), plane)
        rc, text = run_loader(exe, crlf, gw, gh)
        assert rc == 0 and [int(x) for x in text.split()[1:]] == plane.ravel().tolist(), (gw, gh)


ROW = "00ff10"
MALFORMED = [
    ("magic", "mtdir 2\n3 2\n%s\n%s\n" % (ROW, ROW), 1),
    ("no-magic", "3 2\n%s\n%s\n" % (ROW, ROW), 1),
    ("grid", "mtdir 1\n4 2\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-zero", "mtdir 1\n0 2\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-words", "mtdir 1\n3 2 1\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-two-spaces", "mtdir 1\n3  2\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-text", "mtdir 1\n3 x\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-sign", "mtdir 1\n+3 2\n%s\n%s\n" % (ROW, ROW), 2),
    ("grid-long", "mtdir 1\n0000003 2\n%s\n%s\n" % (ROW, ROW), 2),
    ("no-grid", "mtdir 1\n", 2),
    ("short-row", "mtdir 1\n3 2\n%s\n00ff\n" % ROW, 4),
    ("long-row", "mtdir 1\n3 2\n%s01\n%s\n" % (ROW, ROW), 3),
    ("spaced-row", "mtdir 1\n3 2\n00 ff 10\n%s\n" % ROW, 3),
    ("not-hex", "mtdir 1\n3 2\n%s\n0gff10\n" % ROW, 4),
    ("missing-row", "mtdir 1\n3 2\n%s\n" % ROW, 4),
    ("extra-row", "mtdir 1\n3 2\n%s\n%s\n%s\n" % (ROW, ROW, ROW), 5),
    ("blank-line-behind", "mtdir 1\n3 2\n%s\n%s\n\n" % (ROW, ROW), 5),
    ("empty", "", 1),
]


@pytest.mark.parametrize("name, text, line", MALFORMED, ids=[x[0] for x in MALFORMED])
def test_load_plane_rejects_what_the_python_loader_rejects_with_the_line_named(loader, name, text, line):
    exe, d = loader
    path = d / (name + ".mtdir")
    path.write_text(text)
    with pytest.raises(ValueError) as e:
        lanes.load_plane(str(path), (3, 2))
    assert f"line {line}" in str(e.value), str(e.value)
    rc, out = run_loader(exe, path, 3, 2)
    assert rc == 1 and out.startswith("error ") and f"line {line}" in out and out.count("\n") == 0, out


def test_load_plane_names_a_missing_file(loader):
    exe, d = loader
    rc, out = run_loader(exe, d / "none.mtdir", 3, 2)
    assert rc == 1 and "none.mtdir" in out


# ------------------------------------------------------------------ mtgpu_scan_file's usage errors

TOGETHER = "planes are not together with blobs or compensation yet"


@pytest.mark.parametrize("args, text", [
    (["--plane"], "--plane takes the path of a .mtdir file"),
    (["--plane", "p.mtdir", "--allow", "E"], "--plane cannot be combined with --allow: a plane and the allow byte are one rule at two granularities"),
    (["--ignore", "W", "--plane", "p.mtdir"], "--plane cannot be combined with --ignore: a plane and the allow byte are one rule at two granularities"),
    (["--plane", "p.mtdir", "--gmc"], "--plane cannot be combined with --gmc: " + TOGETHER),
    (["--gmc-vectors", "--plane", "p.mtdir"], "--plane cannot be combined with --gmc-vectors: " + TOGETHER),
    (["--plane", "p.mtdir", "--gmc-max-shift", "4"], "--plane cannot be combined with --gmc-max-shift: " + TOGETHER),
    (["--plane", "p.mtdir", "--gmc-min-share-q8", "100"], "--plane cannot be combined with --gmc-min-share-q8: " + TOGETHER),
    (["--plane", "p.mtdir", "--min-blob-cells", "3"], "--plane cannot be combined with --min-blob-cells: " + TOGETHER),
    (["--plane", "p.mtdir", "--sweep-blobs", "3"], "--plane cannot be combined with --sweep-blobs: " + TOGETHER),
    (["--plane", "p.mtdir", "--gmc-blobs", "3"], "--plane cannot be combined with --gmc-blobs: " + TOGETHER),
    (["--sweep-gmc-blobs", "3", "--plane", "p.mtdir"], "--plane cannot be combined with --sweep-gmc-blobs: " + TOGETHER),
    (["--plane", "p.mtdir", "--gmc-blobs-max-shift", "3"], "--plane cannot be combined with --gmc-blobs-max-shift: " + TOGETHER),
    (["--plane", "p.mtdir", "--min-run", "3", "--reach", "2"], "--plane cannot be combined with --reach: " + TOGETHER),
    (["--plane", "p.mtdir", "--dir-sectors", "--centres"], "--dir-sectors cannot be combined with --centres: a pipe has one count array"),
    (["--sweep", "2,3", "--dir-sectors", "--plane", "p.mtdir"], "--dir-sectors cannot be combined with --sweep: a pipe has one count array"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_plane_options_before_any_device_call(args, text):
    """Status 2 and one line naming both options.  Neither the input nor the plane file exists and --streams 0 would ask
    for the device count: the refusal comes before any of them is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "" and out.stderr.count("\n") == 1, out.stderr


@pytest.mark.parametrize("args", [["--plane", "p.mtdir"], ["--plane", "p.mtdir", "--dir-sectors"],
                                  ["--plane", "p.mtdir", "--keep", "k.mtkeep", "--centres", "--sweep", "2"],
                                  ["--plane", "p.mtdir", "--min-run", "3", "--max-dropout", "1"],
                                  ["--plane", "p.mtdir", "--min-blob-cells", "0"]],
                         ids=lambda v: " ".join(v))
def test_scan_file_accepts_what_combines(args):
    """The tool goes on to look for its input."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--threads", "1", "--streams", "1"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 2 and "cannot be combined" not in out.stderr and "takes " not in out.stderr, out.stderr


# ------------------------------------------------------------------ the model against the hand numbers

def test_hand_cases_of_lanes_inputs_by_the_model():
    for name in li.HAND_CASES:
        p, rows = pl.hand_rows(name)
        assert [c for _, _, c, _ in rows] == pl.HAND_DOCUMENTED[name], name
        for f, (fr, plane, want_c, rose) in enumerate(rows):
            fl, ce, wd = pl.model(p, [fr], plane)
            assert ce == [want_c] and fl == [int(want_c >= 1)], (name, f)
            assert wd == [direction.sector_word(rose)], (name, f)
            assert pl.model(p, [fr], plane, np.ones((p.grid_h, p.grid_w), dtype=bool)) == (fl, ce, wd), (name, f)      # P2
    assert [r[3] for r in pl.hand_rows("one_cell")[1]] == [[3, 0, 0, 0, 1, 0, 0, 0]] * 3
    # the margin row: its records do not count, whatever their bytes
    p, rows = pl.hand_rows("margin")
    assert p.vertical_margin == 1 and [direction.unpack_sector_word(pl.model(p, [r[0]], r[1])[2][0]) for r in rows] == [(0x01, 0, 4)] * 2


def test_two_lanes_and_a_clock_by_the_model():
    p, fr, plane, keep, plain, masked = pl.two_lane_case()
    assert plain == (4, 0x15 | 0 << 8 | 2 << 11) and masked == (2, 0x11 | 0 << 8 | 2 << 11)
    fl, ce, wd = pl.model(p, [fr], plane)
    assert (fl, ce[0], wd[0]) == ([1], *plain)
    fl, ce, wd = pl.model(p, [fr], plane, keep)
    assert (fl, ce[0], wd[0]) == ([1], *masked)
    # one byte for the whole picture gives neither pair of numbers
    assert [pd.model(p, [fr], b)[1][0] for b in (0x10, 0xFF)] == [2, 6] and [pd.model(p, [fr], b, keep)[1][0] for b in (0x10, 0xFF)] == [2, 4]
    assert pl.model(p, [fr], pl.filled(p, 0xFF), keep)[2] == [masked[1]] and pl.model(p, [fr], pl.filled(p, 0))[2] == [plain[1]]     # P5


def test_a_filled_plane_is_the_direction_pipe_by_the_models():
    """P3 between the two models, on the shapes case."""
    p, frames, keep, a, b = pl.shapes_case()
    for byte in pl.SHAPE_BYTES:
        assert pl.model(p, frames, pl.filled(p, byte)) == pd.model(p, list(frames), byte), byte
        assert pl.model(p, frames, pl.filled(p, byte), keep) == pd.model(p, list(frames), byte, keep), byte
    assert np.array_equal(a & b, b) and not np.array_equal(a, b)
    for k in (None, keep):                                                     # P6 and P5
        ca, cb = pl.model(p, frames, a, k), pl.model(p, frames, b, k)
        assert all(y <= x for x, y in zip(ca[1], cb[1])) and ca[1] != cb[1] and ca[2] == cb[2]


def test_seams_uhd_pieces_empty_range_and_limit_hand_values_by_the_model():
    for gw in (65, 129):
        fr, planes, hand = pl.seam_rows(gw)
        keep = pd.seam_keep(gw)
        for margin in (0, 1):
            p = pl.seam_params(gw, margin)
            assert [pl.model(p, [fr], pln)[1][0] for pln in planes] == hand == li.SEAM_HAND[gw], (gw, margin)
            assert pl.model(p, [fr], planes[0], keep)[2] == pd.sector_words(p, [fr], keep)
    for vm, staged in ((0.0, 0), (0.05, 1)):
        p, frames, plane, keep = pl.uhd_rows(vm)
        assert m.lanes_preview(p)["staged"] == staged and np.array_equal(plane, li.cellwise_plane(p))
        assert len(frames) == 4 and sum(pl.model(p, frames, plane)[1]) > 0
    assert m.lanes_preview(pl.uhd_rows(0.0)[0])["lds_bytes"] + 240 * 135 > 163840
    p, fr, half, full, keep = pl.pieces_rows()
    assert len(fr) == 300000 > 2 * 131072
    for masked in (False, True):
        k = keep if masked else None
        got = [pl.model(p, [fr], pln, k) for pln in (half, full)]
        assert [g[1][0] for g in got] == pl.PIECES_HAND[masked][0] and [g[2] for g in got] == [[pl.PIECES_HAND[masked][1]]] * 2
    assert direction.unpack_sector_word(pl.PIECES_HAND[False][1]) == (0x08, 3, 300000)
    assert direction.unpack_sector_word(pl.PIECES_HAND[True][1]) == (0x08, 3, 250000)
    p, frames = pl.empty_range_case()
    assert pl.model(p, frames, pl.filled(p, 0xFF)) == ([0] * 3, [0] * 3, [0] * 3) and all(len(f) > 10 for f in frames)
    p, one, two, h1, h2 = pl.stale_case()
    for frames, h in ((one, h1), (two, h2)):
        assert pl.model(p, list(frames), pl.filled(p, 0xFF)) == (h["flags"], h["centres"], h["sectors"])
    shapes = pl.limit_shapes()
    for which, masked in (("staged", False), ("unstaged", False), ("masked", True)):
        gw, gh = shapes[which]
        p = pl.limit_params(gw, gh)
        frames, keep = pl.limit_frames(gw, gh)
        fl, ce, wd = pl.model(p, list(frames), pl.limit_plane(gw, gh), keep if masked else None)
        assert (ce, wd) == pl.LIMIT_HAND[masked] and fl == [1, 1, 0], which


def test_the_limit_shapes_sit_on_their_limits():
    shapes = pl.limit_shapes()
    gw, gh = shapes["staged"]
    assert gw == 65 and m.lanes_preview(dc.grid_params(gw, gh))["staged"] == 1
    assert shapes["unstaged"] == (65, gh + 1) and m.lanes_preview(dc.grid_params(65, gh + 1))["staged"] == 0
    assert m.lanes_preview(dc.grid_params(gw, gh))["lds_bytes"] <= 163840 < m.lanes_preview(dc.grid_params(gw, gh))["lds_bytes"] + 16 + 8 * 65
    zw, zh = shapes["masked"]
    assert (zw, zh) == pd.masked_limit_shape() and zh > gh + 1                   # the mask's limit lies among the unstaged grids
    assert dc.kernel_preview("zones", dc.grid_params(zw, zh)) is not None and dc.kernel_preview("zones", dc.grid_params(zw, zh + 1)) is None
    assert m.lanes_preview(dc.grid_params(zw, zh + 1))["staged"] == 0           # one row further the plane pipe goes on, unmasked
    with pytest.raises(m.MtgpuError) as e:
        m.lanes_preview(m.ScanParams.from_config(3840, 2160, **pl.FINE_KW))
    assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)


# ------------------------------------------------------------------ the model against the oracle, through removal

def oracle_check(p, frames, planes, keep):
    frames = list(frames)
    for i, plane in enumerate(planes):
        assert pl.model(p, frames, plane)[1] == pl.oracle_centres(p, frames, plane), i
        if keep is not None and p.vectors_needed >= 1:
            assert pl.model(p, frames, plane, keep)[1] == pl.oracle_centres(p, frames, plane, keep), i
    if keep is not None:
        assert pl.sector_words(p, frames, np.ones_like(keep)) == pl.sector_words(p, frames)


def test_model_agrees_with_the_oracle_on_the_fixed_inputs():
    for name in li.HAND_CASES:
        p, rows = pl.hand_rows(name)
        for fr, plane, _, _ in rows:
            oracle_check(p, [fr], [plane], None)
    p, fr, plane, keep, _, _ = pl.two_lane_case()
    oracle_check(p, [fr], [plane, pl.filled(p, 0xFF)], keep)
    p, frames, keep, a, b = pl.shapes_case()
    oracle_check(p, frames, [a, b] + [pl.filled(p, x) for x in pl.SHAPE_BYTES], keep)
    for gw in (65, 129):
        fr, planes, _ = pl.seam_rows(gw)
        for margin in (0, 1):
            oracle_check(pl.seam_params(gw, margin), [fr], planes, pd.seam_keep(gw))
    for vm in (0.0, 0.05):
        p, frames, plane, keep = pl.uhd_rows(vm)
        oracle_check(p, frames, [plane], keep)
    e = di.edge_case()
    oracle_check(e["params"], pd.case_frames(e), [li.cellwise_plane(e["params"])], None)
    p, fr, half, full, keep = pl.pieces_rows()
    oracle_check(p, [fr], [half, full], keep)
    p, frames = pl.empty_range_case()
    oracle_check(p, frames, [pl.filled(p, 0xFF)], None)
    for which in ("staged", "unstaged", "masked"):
        gw, gh = pl.limit_shapes()[which]
        frames, keep = pl.limit_frames(gw, gh)
        oracle_check(pl.limit_params(gw, gh), frames, [pl.limit_plane(gw, gh)], keep)


@pytest.mark.parametrize("i", range(pl.N_DRAWS))
def test_model_agrees_with_the_oracle_on_the_draws(i):
    p, frames, keep, chain = pl.draw(i)
    assert len(chain) == 5 and m.lanes_preview(p)
    for lo, hi in zip(chain, chain[1:]):
        assert np.array_equal(lo & hi, lo)
    oracle_check(p, frames, chain[1:4], keep)
    # the model's removal is lanes_model.filter_records' rule
    fr = next(f for f in frames if f is not None)
    assert np.array_equal(pl.remove_forbidden(p, [fr], chain[2])[0], fr[lm.allowed(p, fr, chain[2])])


def test_the_recording_by_the_model():
    p, frames, pts, keep, hand = pl.recording_case()
    frames = list(frames)
    b = m.FrameBatch.from_frames(frames)
    flow = lm.flow_map(p, b.mv, b.frame_off, None, np.array([0, pl.REC_FRAMES], dtype=np.uint64))[0]
    plane = lanes.plane_from_flow(flow, 4, 102, 1, 0xFF)                       # --min-records 4 --share 0.4 --widen 1
    assert np.array_equal(plane, hand)
    wrong = lanes.invert_plane(plane, plane != 0xFF, 0)
    assert all(wrong[y, x] == 0xFF for x, y in pl.CLOCK) and wrong[2, 5] == 0xC7 and wrong[7, 5] == 0x7C and wrong[0, 0] == 0
    assert pl.model(p, frames, wrong)[0] == [1] * pl.REC_FRAMES                # the clock alone flags every frame
    fl, ce, wd = pl.model(p, frames, wrong, keep)
    assert [f for f in range(pl.REC_FRAMES) if fl[f]] == pl.AGAINST == list(range(40, 50)) + list(range(60, 70))
    oracle_check(p, frames, [wrong, plane], keep)
    # the words under the mask: the 30 + 10 + 10 + 10 frames with an object
    assert pl.recording_stats(wd) == (60, [50, 0, 0, 0, 50, 0, 0, 0], [50, 0, 0, 0, 10, 0, 0, 0])
