"""CPU tier: what the direction filter through the pipe (include/mtgpu_pipe_dir.h) promises without a device — the ABI,
the header, the refusals that come before any HIP call, the sector word in pure Python — and the inputs and the model of
tests/test_gpu_pipe_dir.py: every hand-derived number against the model, the model against the unchanged oracle through
removal on every input, and the preview facts the limit cases rest on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction

import derived_cliff_inputs as dc
import dir_inputs as di
import dir_model as dm
import pipe_dir_inputs as pd
import pipe_gmc_inputs as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)


# ------------------------------------------------------------------ the ABI and the sources

def test_abi_declares_what_the_header_declares_and_the_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "mtgpu_pipe_dir.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", text))) == sorted(_abi.ABI_PIPE_DIR) == ["mtgpu_pipe_dir", "mtgpu_pipe_set_dir"]
    lib = m.load_library()
    for n in _abi.ABI_PIPE_DIR:
        assert hasattr(lib, n)
    assert '#include "mtgpu_pipe_dir.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert re.search(r"#define MT_PIPE_REPORT_SECTORS 3\b", text) and _abi.MT_PIPE_REPORT_SECTORS == 3
    assert _abi.MT_PIPE_REPORT_SECTORS not in (_abi.MT_PIPE_REPORT_CENTRES, _abi.MT_PIPE_REPORT_LARGEST, _abi.MT_PIPE_REPORT_VECTOR)


def test_null_pipe_is_refused_without_a_device():
    lib = m.load_library()
    assert lib.mtgpu_pipe_set_dir(None, 1, 0xFF, 0) == _abi.MT_ERR_INVALID and b"pipe is NULL" in lib.mtgpu_last_error()
    assert lib.mtgpu_pipe_set_dir(None, 0, 0, 0) == _abi.MT_ERR_INVALID
    a = C.c_int32(7)
    assert lib.mtgpu_pipe_dir(None, C.byref(a), None) == -1 and a.value == 7


def test_both_forms_of_the_kernel_are_in_the_library_and_the_pipe_reads_no_new_environment():
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        for pipe in (0, 1):
            assert b"dir_frames_kernelILi1024ELi4ELi%dELb%dEE" % (rec, pipe) in blob, (rec, pipe)
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    assert pipe_src.count("getenv") == 4
    assert "getenv" not in open(os.path.join(PKG, "csrc", "dir_kernels.hip")).read()
    # which scan a submit runs is the pipe's ONE mode (csrc/pipe_mode.h), so there is no order of tests left to hold: that no
    # second mode can be on next to this one is held by cases (a) and (b) of tests/golden/pipe_mode_matrix.json, recorded from
    # the commit before the modes became one value, together with this mode's result tests (tests/test_gpu_pipe_dir.py)
    import pipe_mode_matrix as pm
    assert pm.excludes_every_other("dir")


def test_header_compiles_alone_as_c11_and_as_cpp17(tmp_path):
    body = ("int use(mtgpu_pipe *p) {\n  int32_t a = 0;\n  int r = 0;\n"
            "  return mtgpu_pipe_set_dir(p, 1, 0xFF, MT_PIPE_REPORT_SECTORS) + mtgpu_pipe_set_dir(p, 0, 0, MT_PIPE_REPORT_CENTRES)\n"
            "       + mtgpu_pipe_dir(p, &a, &r) + mtgpu_pipe_dir(p, 0, 0) + (int)a + r;\n}\n")
    for first in ("mtgpu_pipe_dir.h", "mtgpu.h", "mtgpu_dir.h", "mtgpu_pipe_gmc.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_dir.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_dir) and callable(m.ScanPipe.clear_dir) and callable(m.ScanPipe.dir)
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_dir(int allow)", "void report_sectors(bool on)", "int dir_allow = -1;", "bool dir_sectors = false;",
                 "uint64_t dir_present_frames[8]", "uint64_t dir_dominant_frames[8]", "inline DirOptions &dir_options()",
                 "scanners[i]->report_sectors(out.dir_sectors)"):
        assert text in host, text
    # initialize() turns every mode off before it settles this video's one (all_off): held on a GPU by the 36 "the previous
    # video ran X, this video asks Y" pairs of tests/test_gpu_host_mode_matrix.py
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    for opt in ('"--allow"', '"--ignore"', '"--dir-sectors"'):
        assert opt in tool


def test_plain_c_example_and_the_host_program_compile():
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_dir_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_dir_two_videos.cpp")])


def test_set_dir_refuses_a_bad_report_before_any_call():
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)
    pipe = m.ScanPipe.__new__(m.ScanPipe)
    pipe._lib, pipe._pipe = NoLibrary(), None
    for report in ("vector", "largest", "rose", "", None, 3):
        with pytest.raises(ValueError):
            pipe.set_dir(0xFF, report)
    with pytest.raises(ValueError):
        pipe.set_dir("E,XX")                                                   # allow_from_names' refusal, before any call too
    pipe._pipe = None                                                          # (close() finds nothing to destroy)


# ------------------------------------------------------------------ the sector word

def test_sector_word_and_its_unpacking():
    sw, un = direction.sector_word, direction.unpack_sector_word
    w = sw([2, 2, 1, 0, 0, 0, 0, 0])
    assert w == 0x07 | (0 << 8) | (2 << 11) == pd.BOUNDARY_WORD and un(w) == (0x07, 0, 2)      # the tie goes to the smallest k
    assert sw([0] * 8) == 0 and un(0) == (0, None, 0)
    big = 1 << 21
    assert un(sw([0, 0, 0, 0, 0, 0, 0, big])) == (0x80, 7, big - 1)                            # saturated
    assert un(sw([0, 0, 0, 0, 0, 0, 0, big - 1])) == (0x80, 7, big - 1)                        # the largest exact count
    assert un(sw([0, 0, 0, 0, 0, 0, 0, big - 2])) == (0x80, 7, big - 2)
    assert sw([0, 0, 0, 0, 0, 0, 0, 1 << 40]) == 0x80 | (7 << 8) | ((big - 1) << 11) == 0xFFFFFF80
    assert un(sw([1, 0, 5, 0, 5, 0, 0, 3])) == (0x95, 2, 5)                                    # the first of two maxima
    assert un(sw(np.array([1] * 8, dtype=np.uint32))) == (0xFF, 0, 1)
    for bad in ([1] * 7, [1] * 9, [-1] + [0] * 7):
        with pytest.raises(ValueError):
            sw(bad)
    with pytest.raises(ValueError):
        un(1 << 32)
    assert pd.word(0x10, 4, 2) == sw([0, 0, 0, 0, 2, 0, 0, 0])


# ------------------------------------------------------------------ mtgpu_scan_file's usage errors

TOGETHER = "direction is not together with blobs or compensation yet"
LIST = "takes a comma-separated list of sector names (E,SE,S,SW,W,NW,N,NE) or one decimal number in [0, 255]"


@pytest.mark.parametrize("args, text", [
    (["--allow", "E", "--ignore", "W"], "--allow cannot be combined with --ignore"),
    (["--ignore", "W", "--allow", "E"], "--allow cannot be combined with --ignore"),
    (["--allow"], "--allow " + LIST),
    (["--ignore"], "--ignore " + LIST),
    (["--allow", "E,Q"], "--allow " + LIST),
    (["--allow", "E,"], "--allow " + LIST),
    (["--allow", ""], "--allow " + LIST),
    (["--ignore", "256"], "--ignore " + LIST),
    (["--ignore", "12x"], "--ignore " + LIST),
    (["--ignore", "0x11"], "--ignore " + LIST),
    (["--allow", "E", "--gmc"], "--allow cannot be combined with --gmc: " + TOGETHER),
    (["--gmc-vectors", "--ignore", "W"], "--ignore cannot be combined with --gmc-vectors: " + TOGETHER),
    (["--dir-sectors", "--gmc-max-shift", "4"], "--dir-sectors cannot be combined with --gmc-max-shift: " + TOGETHER),
    (["--allow", "E", "--min-blob-cells", "3"], "--allow cannot be combined with --min-blob-cells: " + TOGETHER),
    (["--allow", "E", "--sweep-blobs", "3"], "--allow cannot be combined with --sweep-blobs: " + TOGETHER),
    (["--allow", "E", "--gmc-blobs", "3"], "--allow cannot be combined with --gmc-blobs: " + TOGETHER),
    (["--ignore", "N", "--sweep-gmc-blobs", "3"], "--ignore cannot be combined with --sweep-gmc-blobs: " + TOGETHER),
    (["--ignore", "N", "--gmc-blobs-max-shift", "3"], "--ignore cannot be combined with --gmc-blobs-max-shift: " + TOGETHER),
    (["--allow", "E", "--min-run", "3", "--reach", "2"], "--allow cannot be combined with --reach: " + TOGETHER),
    (["--dir-sectors", "--centres"], "--dir-sectors cannot be combined with --centres: a pipe has one count array"),
    (["--sweep", "2,3", "--dir-sectors", "--allow", "E"], "--dir-sectors cannot be combined with --sweep: a pipe has one count array"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_dir_options_before_any_device_call(args, text):
    """Status 2 and one line naming both options.  The input does not exist and --streams 0 would ask for the device
    count: the refusal comes before either is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "" and out.stderr.count("\n") == 1, out.stderr


@pytest.mark.parametrize("args", [["--allow", "e,sw"], ["--ignore", "017"], ["--allow", "255", "--centres", "--sweep", "2"],
                                  ["--dir-sectors", "--min-run", "3", "--max-dropout", "1"], ["--allow", "E", "--min-blob-cells", "0"],
                                  ["--allow", "E", "--allow", "W"]],
                         ids=lambda v: " ".join(v))
def test_scan_file_accepts_what_combines(args):
    """The tool goes on to look for its input."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--threads", "1", "--streams", "1"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode != 2 and "cannot be combined" not in out.stderr and "takes a" not in out.stderr, out.stderr


# ------------------------------------------------------------------ the model against the hand numbers

def test_hand_cases_of_dir_inputs_by_the_model():
    for name, make in di.HAND_CASES.items():
        case = make()
        p, frames, allows = case["params"], pd.case_frames(case), pd.case_allows(case)
        for f, (fr, a) in enumerate(zip(frames, allows)):
            fl, ce, wd = pd.model(p, [fr], a)
            assert ce == [int(case["hand_centres"][f])], (name, f)
            assert wd == [direction.sector_word(case["hand_rose"][f])], (name, f)
    b = di.boundary_case()
    assert b["hand_centres"].tolist() == [5, 0, 4, 0, 2, 0] and pd.case_allows(b) == di.BOUNDARY_ALLOWS
    fr = pd.case_frames(b)[0]
    assert {tuple(pd.model(b["params"], [fr], a)[2]) for a in di.BOUNDARY_ALLOWS} == {(pd.BOUNDARY_WORD,)}         # D5
    v = di.vn0_case()
    assert [pd.model(v["params"], [pd.case_frames(v)[0]], a)[1] for a in (0, 0x10, 0xFF)] == [[20]] * 3


def test_mask_hand_frames_by_the_model():
    spelled = {"a": ((2, 0x10 | 4 << 8 | 2 << 11), (5, 0x11 | 0 << 8 | 6 << 11)),
               "b": ((19, 0x07 | 2 << 11), (20, 0x07 | 2 << 11)), "b0": ((19, 0), (20, 0)),
               "c": ((1, 0x11 | 2 << 11), (2, 0x11 | 3 << 11)), "c-all": ((3, 0x11 | 2 << 11), (4, 0x11 | 3 << 11))}
    h = pd.mask_hand()
    assert {k: (v[4], v[5]) for k, v in h.items()} == spelled
    for name, (p, fr, keep, allow, masked, plain) in h.items():
        fl, ce, wd = pd.model(p, [fr], allow, keep)
        assert (ce[0], wd[0]) == masked and fl == [int(masked[0] >= 1)], name
        fl, ce, wd = pd.model(p, [fr], allow)
        assert (ce[0], wd[0]) == plain, name
        assert pd.model(p, [fr], allow, np.ones((5, 6), dtype=bool)) == pd.model(p, [fr], allow), name          # D2
    # a mask that reaches only the active plane would report frame a's six E records
    p, fr, keep = h["a"][:3]
    assert direction.unpack_sector_word(pd.sector_words(p, [fr])[0]) == (0x11, 0, 6)
    assert direction.unpack_sector_word(pd.sector_words(p, [fr], keep)[0]) == (0x10, 4, 2)


def test_seams_big_frame_stale_and_limit_hand_values_by_the_model():
    for gw in (65, 129):
        case = di.seam_case(gw)
        fr, keep = pd.case_frames(case)[0], pd.seam_keep(gw)
        assert [pd.model(case["params"], [fr], a)[1][0] for a in di.SEAM_ALLOWS] == di.SEAM_HAND[gw]
        assert [pd.model(case["params"], [fr], a, keep)[1][0] for a in di.SEAM_ALLOWS] == pd.SEAM_MASKED_HAND[gw] == \
            {65: [4, 1, 0], 129: [8, 2, 0]}[gw]
    p, big = pd.big_case()
    assert len(big) == 262145 == 2 * 131072 + 1
    assert pd.sector_words(p, [big]) == [pd.BIG_WORD] and direction.unpack_sector_word(pd.BIG_WORD) == (0xFF, 3, 262138)
    p, one, two, h1, h2 = pd.stale_case()
    for frames, h in ((one, h1), (two, h2)):
        assert pd.model(p, list(frames), 0xFF) == (h["flags"], h["centres"], h["sectors"])
    assert (h1, h2) == ({"flags": [1] * 3, "centres": [5] * 3, "sectors": [0x07 | 2 << 11] * 3},
                        {"flags": [1, 0, 0], "centres": [4, 0, 0], "sectors": [0x11 | 3 << 11, 0x01 | 1 << 11, 0]})
    for shape, masked in ((pd.limit_shape(), False), (pd.masked_limit_shape(), True)):
        gw, gh = shape
        p = pd.limit_params(gw, gh)
        frames, keep = pd.limit_frames(gw, gh)
        for a, want in zip(pd.LIMIT_ALLOWS, pd.LIMIT_HAND[masked][0]):
            fl, ce, wd = pd.model(p, list(frames), a, keep if masked else None)
            assert ce == want and fl == [int(c >= 2) for c in want] and wd == pd.LIMIT_HAND[masked][1], (shape, a)


def test_the_limit_shapes_sit_on_their_limits():
    gw, gh = pd.limit_shape()
    assert gw == 65 and dc.kernel_preview("zones", dc.grid_params(gw, gh)) is None                  # only mtgpu_dir_preview accepts it
    assert m.dir_preview(dc.grid_params(gw, gh))["lds_bytes"] <= 163840
    with pytest.raises(m.MtgpuError) as e:
        m.dir_preview(dc.grid_params(gw, gh + 1))
    assert e.value.code == _abi.MT_ERR_UNSUPPORTED and f"{gw}x{gh + 1}" in str(e.value)
    zw, zh = pd.masked_limit_shape()
    assert zw == 65 and zh < gh
    assert dc.kernel_preview("zones", dc.grid_params(zw, zh)) is not None and dc.kernel_preview("zones", dc.grid_params(zw, zh + 1)) is None
    assert m.dir_preview(dc.grid_params(zw, zh)) and (zw, zh) == dc.shapes("zones")[f"tall-65x{zh}"][:2]
    with pytest.raises(m.MtgpuError) as e:
        m.dir_preview(m.ScanParams.from_config(3840, 2160, **pd.FINE_KW))
    assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)


# ------------------------------------------------------------------ the model against the oracle, through removal

def oracle_check(p, frames, allows, keep):
    frames = list(frames)
    for a in allows:
        assert pd.model(p, frames, a)[1] == pd.oracle_centres(p, frames, a), a
        if keep is not None and p.vectors_needed >= 1:
            assert pd.model(p, frames, a, keep)[1] == pd.oracle_centres(p, frames, a, keep), a
    # the rose behind the word: dir_model's, on the frames without their keep-0 records; D5 is built in (no allow argument)
    if keep is not None:
        ones = np.ones_like(keep)
        assert pd.sector_words(p, frames, ones) == pd.sector_words(p, frames)


def test_model_agrees_with_the_oracle_on_the_fixed_inputs():
    for make in di.HAND_CASES.values():
        case = make()
        oracle_check(case["params"], pd.case_frames(case), sorted(set(pd.case_allows(case))), None)
    for p, fr, keep, allow, _, _ in pd.mask_hand().values():
        oracle_check(p, [fr], [allow, 0xFF], keep)
    p, frames, keep = pd.shapes_case()
    oracle_check(p, frames, pd.SHAPE_ALLOWS, keep)
    for gw in (65, 129):
        case = di.seam_case(gw)
        oracle_check(case["params"], pd.case_frames(case)[:1], di.SEAM_ALLOWS, pd.seam_keep(gw))
    e = di.edge_case()
    oracle_check(e["params"], pd.case_frames(e), [di.EDGE_ALLOW], None)
    p, big = pd.big_case()
    oracle_check(p, [big], [0xFF, 0xF7], None)
    p, one, two, _, _ = pd.stale_case()
    oracle_check(p, list(one) + list(two), [0xFF], None)
    for shape in (pd.limit_shape(), pd.masked_limit_shape()):
        frames, keep = pd.limit_frames(*shape)
        oracle_check(pd.limit_params(*shape), frames, pd.LIMIT_ALLOWS, keep)
    p, frames, _, keep = pd.recording_case()
    oracle_check(p, frames, [0xFF, 0xC7, 0x7C], keep)


@pytest.mark.parametrize("i", range(pd.N_DRAWS))
def test_model_agrees_with_the_oracle_on_the_draws(i):
    p, frames, keep = pd.draw(i)
    assert 1 <= len(frames) <= 12 and max(len(f) for f in frames if f is not None) <= 3000 and frames[0] is not None
    assert p.vectors_needed == i % 4 and dc.kernel_preview("zones", p) is not None and m.dir_preview(p)
    oracle_check(p, frames, pd.DRAW_ALLOWS, keep)


def test_the_draws_cover_what_they_are_for():
    seen_vn, seen_margin, seen_none, shares = set(), set(), 0, set()
    for i in range(pd.N_DRAWS):
        p, frames, keep = pd.draw(i)
        seen_vn.add(p.vectors_needed), seen_margin.add(p.vertical_margin)
        seen_none += sum(f is None for f in frames)
        shares.add(min((0.05, 0.3, 0.7), key=lambda s: abs(s - (1.0 - float(keep.mean())))))
    assert seen_vn == {0, 1, 2, 3} and {0, 1, 2, 3} <= seen_margin and seen_none >= 5 and shares == {0.05, 0.3, 0.7}


def test_the_recording_by_the_model():
    p, frames, pts, keep = pd.recording_case()
    sd = [f is not None for f in frames]
    every = [int(s) for s in sd]
    assert pd.model(p, list(frames), 0xFF)[0] == every and pd.model(p, list(frames), 0xC7)[0] == every           # the clock flags every frame
    east = pd.model(p, list(frames), direction.allow_from_names("E,SE,S,N,NE"), keep)[0]
    west = pd.model(p, list(frames), direction.allow_from_names("S,SW,W,NW,N"), keep)[0]
    assert [f for f in range(pd.REC_FRAMES) if east[f]] == list(pd.EAST) and [f for f in range(pd.REC_FRAMES) if west[f]] == list(pd.WEST)
    words = pd.sector_words(p, list(frames), keep)
    assert pd.recording_stats(words) == (16, [10, 0, 0, 0, 6, 0, 0, 0], [10, 0, 0, 0, 6, 0, 0, 0])
    assert pd.recording_stats(pd.sector_words(p, list(frames)))[0] == 38
