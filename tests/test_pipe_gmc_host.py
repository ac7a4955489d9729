"""CPU tier: what global-motion compensation through the pipe (include/mtgpu_pipe_gmc.h) promises without a device — the
ABI, the headers, the refusals that come before any HIP call — and the inputs and the model of tests/test_gpu_pipe_gmc.py:
the hand frames against their hand-derived values, P2 - P4 inside the model, the preview facts the limit cases rest on,
and the packing of the vector report."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_cliff_inputs as dc
import gmc_model as gm
import pipe_gmc_inputs as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)


# ------------------------------------------------------------------ the ABI and the sources

def test_abi_declares_what_the_header_declares():
    text = open(os.path.join(ROOT, "include", "mtgpu_pipe_gmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", text))) == sorted(_abi.ABI_PIPE_GMC) == ["mtgpu_pipe_gmc", "mtgpu_pipe_set_gmc"]
    lib = m.load_library()
    for n in _abi.ABI_PIPE_GMC:
        assert hasattr(lib, n)
    assert '#include "mtgpu_pipe_gmc.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert re.search(r"#define MT_PIPE_REPORT_VECTOR 2\b", text) and _abi.MT_PIPE_REPORT_VECTOR == 2
    assert _abi.MT_PIPE_REPORT_VECTOR not in (_abi.MT_PIPE_REPORT_CENTRES, _abi.MT_PIPE_REPORT_LARGEST)


def test_null_pipe_is_refused_without_a_device():
    lib = m.load_library()
    assert lib.mtgpu_pipe_set_gmc(None, 1, 16, 128, 0) == _abi.MT_ERR_INVALID and b"pipe is NULL" in lib.mtgpu_last_error()
    assert lib.mtgpu_pipe_set_gmc(None, 0, 0, 0, 0) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_pipe_gmc(None, None, None, None) == -1
    a = C.c_int32(7)
    assert lib.mtgpu_pipe_gmc(None, C.byref(a), None, None) == -1 and a.value == 7


def test_both_forms_of_the_kernel_are_in_the_library_and_the_pipe_reads_no_new_environment():
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        for pipe in (0, 1):
            assert b"gmc_frames_kernelILi1024ELi4ELi%dELb%dEE" % (rec, pipe) in blob, (rec, pipe)
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    assert pipe_src.count("getenv") == 4
    assert "getenv" not in open(os.path.join(PKG, "csrc", "gmc_kernels.hip")).read()
    # which scan a submit runs is the pipe's ONE mode (csrc/pipe_mode.h), so there is no order of tests left to hold: that no
    # second mode can be on next to this one is held by cases (a) and (b) of tests/golden/pipe_mode_matrix.json, recorded from
    # the commit before the modes became one value, together with this mode's result tests (tests/test_gpu_pipe_gmc.py)
    import pipe_mode_matrix as pm
    assert pm.excludes_every_other("gmc")


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_pipe *p) {\n  int32_t a = 0, b = 0;\n  int r = 0;\n"
            "  return mtgpu_pipe_set_gmc(p, 1, MTGPU_GMC_DEFAULT_MAX_SHIFT, MTGPU_GMC_DEFAULT_MIN_SHARE_Q8, MT_PIPE_REPORT_VECTOR)\n"
            "       + mtgpu_pipe_set_gmc(p, 0, 0, 0, MT_PIPE_REPORT_CENTRES) + mtgpu_pipe_gmc(p, &a, &b, &r) + mtgpu_pipe_gmc(p, 0, 0, 0)\n"
            "       + (int)a + (int)b + r + MT_PIPE_REPORT_LARGEST;\n}\n")
    for first in ("mtgpu.h", "mtgpu_pipe_gmc.h", "mtgpu_gmc.h", "mtgpu_pipe_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_gmc.h"\n#include "mtgpu_pipe_blobs.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_gmc) and callable(m.ScanPipe.clear_gmc) and callable(m.ScanPipe.gmc)
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_gmc(int max_shift, int min_share_q8", "void report_vector(bool on)", "int gmc_max_shift = -1;",
                 "bool gmc_vectors = false;", "inline GmcOptions &gmc_options()", "scanners[i]->report_vector(out.gmc_vectors)"):
        assert text in host, text
    tool = open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()
    for opt in ('"--gmc"', '"--gmc-max-shift"', '"--gmc-min-share-q8"', '"--gmc-vectors"'):
        assert opt in tool


def test_plain_c_example_and_the_host_program_compile():
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_gmc_example.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_gmc_two_videos.cpp")])


BLOBS = "--gmc cannot be combined with --min-blob-cells or --sweep-blobs"
COUNTS = "--gmc-vectors cannot be combined with --centres or --sweep"


@pytest.mark.parametrize("args, text", [
    (["--gmc", "--min-blob-cells", "3"], BLOBS),
    (["--min-blob-cells", "3", "--gmc-max-shift", "4"], BLOBS),
    (["--gmc-min-share-q8", "64", "--sweep-blobs", "8"], BLOBS),
    (["--gmc-vectors", "--sweep-blobs", "8"], BLOBS),
    (["--gmc-vectors", "--centres"], COUNTS),
    (["--sweep", "2,3", "--gmc-vectors"], COUNTS),
    (["--gmc-max-shift", "128"], "--gmc-max-shift takes an integer in [0, 127]"),
    (["--gmc-max-shift", "-1"], "--gmc-max-shift takes an integer in [0, 127]"),
    (["--gmc-max-shift", "4x"], "--gmc-max-shift takes an integer in [0, 127]"),
    (["--gmc-max-shift"], "--gmc-max-shift takes an integer in [0, 127]"),
    (["--gmc-min-share-q8", "257"], "--gmc-min-share-q8 takes an integer in [0, 256]"),
    (["--gmc-min-share-q8"], "--gmc-min-share-q8 takes an integer in [0, 256]"),
], ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_scan_file_refuses_bad_gmc_options_before_any_device_call(args, text):
    """Status 2 and a message naming the option.  The input does not exist and --streams 0 would ask for the device
    count: the refusal comes before either is looked at."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--streams", "0"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and text in out.stderr and out.stdout == "", out.stderr


def test_min_blob_cells_zero_next_to_gmc_is_no_conflict():
    """--min-blob-cells 0 is "off": the tool goes on to look for its input."""
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "does_not_exist.mtmv", "--threads", "1", "--streams", "1", "--gmc", "--min-blob-cells", "0"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode != 2 and "cannot be combined" not in out.stderr


# ------------------------------------------------------------------ the hand frames, by the model

def test_hand_frames_against_the_model_with_their_values_spelled_out():
    p = pg.params()
    h = pg.hand_frames()
    assert [len(h[k]) for k in "abcde"] == [4800, 4800, 4860, 240, 16]
    spelled = {
        "a-plain": (1, 2360, None), "a-gmc": (0, 0, (9, 3)), "b-gmc": (1, 4, (9, 3)),
        "c-gmc-no-mask": (1, 30, (9, 3)), "c-gmc-mask": (0, 0, (9, 3)),
        "d-plain": (1, 40, None), "d-gmc-no-mask": (1, 40, (0, 0)), "d-gmc-mask": (0, 0, (9, 3)),
        "e-gmc-mask": (1, 2, (9, 3)), "e-gmc-ones": (1, 4, (0, 0)), "e-gmc-no-mask": (1, 4, (0, 0)),
    }
    assert {n: v for n, _, _, _, v in pg.HAND} == spelled
    for name, fr, kp, mode, (flag, centres, vec) in pg.HAND:
        keep = pg.KEEPS[kp]
        if mode == "plain":
            assert pg.masked_plain(p, [h[fr]], keep) == ([flag], [centres]), name
        else:
            assert pg.model(p, [h[fr]], pg.MS, pg.Q8, keep) == ([flag], [centres], [pg.pack_vector(*vec)]), name
    # the estimates behind them: (gx, gy, n_in, mode_x, n_x, mode_y, n_y)
    assert pg.estimate(p, h["b"], 16, 128) == (9, 3, 4800, 9, 4792, 3, 4800)
    assert pg.estimate(p, h["c"], 16, 128) == (9, 3, 4860, 9, 4800, 3, 4800)
    assert pg.estimate(p, h["c"], 16, 128, pg.KEEP_C) == (9, 3, 4800, 9, 4800, 3, 4800)
    assert pg.estimate(p, h["d"], 16, 128) == (0, 0, 240, 0, 160, 0, 160)
    assert pg.estimate(p, h["d"], 16, 128, pg.KEEP_D) == (9, 3, 80, 9, 80, 3, 80)
    assert pg.estimate(p, h["e"], 16, 128, pg.KEEP_E) == (9, 3, 8, 9, 4, 3, 4) and 4 * 256 >= 128 * 8
    assert pg.estimate(p, h["e"], 16, 128, pg.ONES) == (0, 0, 16, 0, 8, 0, 8) and 4 * 256 < 128 * 16
    # a mask that reached only the active plane would leave d's mode at 0: the 40 centres stay
    assert pg.residual_centres(p, h["d"], 0, 0, pg.KEEP_D) == 40
    # without a keep plane the model is tests/gmc_model.py
    for k in "abcde":
        c, info = gm.gmc_frame(p, h[k], 16, 128)
        assert pg.model(p, [h[k]], 16, 128) == ([int(c >= 2)], [c], [pg.pack_vector(info["gx"], info["gy"])])


def test_p2_p3_p4_inside_the_model():
    p, frames, keep = pg.shapes_case()
    assert frames[0] is None and frames[3] is None and frames[-1] is None and len(frames[5]) == 0 and len(frames[12]) == 1
    assert all(f is None or f.dtype.itemsize == 40 for f in frames)
    small = [f for f in frames if f is None or len(f) < 10000] + [frames[1]]
    for ms, q8 in pg.SETTINGS:
        none, ones, masked = (pg.model(p, small, ms, q8, k) for k in (None, pg.ONES, keep))
        assert none == ones                                                        # P2
        if ms == 0:                                                                # P3
            assert (none[0], none[1]) == pg.masked_plain(p, small) and (masked[0], masked[1]) == pg.masked_plain(p, small, keep)
            assert set(none[2]) == {0}
            continue
        for f, c, v in zip(small, masked[1], masked[2]):                           # P4
            if f is None:
                continue
            info = gm.estimate(p, pg.remove_masked(p, f, keep), ms, q8)
            assert pg.pack_vector(info["gx"], info["gy"]) == v
            moved = pg.shifted(f, info["gx"], info["gy"])
            assert moved is not None and pg.masked_plain(p, [moved], keep)[1] == [c]
    # the mask matters in this batch, for the estimate and for the plane
    a, b = pg.model(p, small, 16, 128), pg.model(p, small, 16, 128, keep)
    assert a[1] != b[1] and a[2] != b[2]


def test_stale_limit_and_recording_inputs_do_what_the_gpu_cases_need():
    p, one, two, h1, h2 = pg.stale_case()
    m1, m2 = pg.model(p, one, pg.MS, pg.Q8), pg.model(p, two, pg.MS, pg.Q8)
    assert m1 == (h1["flags"], h1["centres"], h1["vector"]) and m2 == (h2["flags"], h2["centres"], h2["vector"])
    assert not set(zip(*m1)) & set(zip(*m2))                                      # every slot changes
    p, frames, pts, keep = pg.recording_case()
    plain, comp, both = pg.masked_plain(p, frames)[0], pg.model(p, frames, 16, 128)[0], pg.model(p, frames, 16, 128, keep)[0]
    assert plain == comp and sum(comp) == 27                                      # the overlay keeps every moving frame flagged
    assert both == [int(10 <= f < 20) for f in range(pg.REC_FRAMES)]
    assert pg.masked_plain(p, frames, keep)[0] == plain                           # the mask alone does not help either
    assert len({v for v in pg.model(p, frames, 16, 128, keep)[2]}) > 8            # more vectors than --gmc-vectors prints


def test_preview_facts_of_the_limit_cases():
    """Every limit shape of the compensated scan is rejected by the masked scan (its layout holds R more keep rows and a
    second plane); the masked scan's limit shapes are accepted by the compensated scan; gmc_lds_bytes has not moved."""
    shapes = dc.shapes("gmc")
    assert sorted(shapes) == sorted(["tall-2x10108", "tall-3x8086", "tall-65x584", "tall-193x199", "wide-13069x1", "wide-7841x3"])
    for name, (gw, gh, kind) in shapes.items():
        p = dc.grid_params(gw, gh)
        pv = dc.kernel_preview("gmc", p)
        assert pv is not None and pv["lds_bytes"] == dc.lds_need("gmc", gw, gh) <= dc.MI355X_LDS, name
        assert dc.kernel_preview("gmc", dc.grid_params(*dc.one_more(gw, gh, kind))) is None, name
        assert dc.kernel_preview("zones", p) is None, name
    gw, gh, _ = shapes["tall-65x584"]
    assert dc.lds_need("zones", gw, gh) - dc.lds_need("gmc", gw, gh) > 15000      # "about 16 KB more"
    for name, (gw, gh, _) in dc.shapes("zones").items():
        assert dc.kernel_preview("gmc", dc.grid_params(gw, gh)) is not None, name
    with pytest.raises(m.MtgpuError) as e:
        m.gmc_preview(m.ScanParams.from_config(3840, 2160, **pg.FINE_KW), dc.MI355X_LDS)
    assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
    # the limit frames' hand values
    for (gw, gh), keep_it, want in (((65, 584), False, [0, 2, 2, 0]), ((65, 530), True, [0, 2, 0, 0])):
        p = dc.grid_params(gw, gh, vectors_needed=1, mv_threshold_sq=16.0, clusters_needed=2)
        clear = [(1, gh // 2), (2, gh // 2)]
        keep = None
        if keep_it:
            keep = np.ones((gh, gw), dtype=bool)
            for x, y in clear:
                keep[y, x] = False
        fl, ce, ve = pg.model(p, pg.limit_frames(gw, gh, dc.shift_of(gw, gh), clear), 16, 128, keep)
        assert ce == want and ve == [pg.pack_vector(7, -3)] * 3 + [0]


def test_packing_of_the_vector_report():
    assert pg.pack_vector(9, 3) == 9 | 3 << 16 == 196617
    assert pg.pack_vector(-9, -3) == 0xFFF7 | 0xFFFD << 16 and pg.pack_vector(7, -3) == 7 | 0xFFFD << 16
    assert pg.pack_vector(-127, 127) == 0xFF81 | 127 << 16 and pg.pack_vector(0, -1) == 0xFFFF0000
    for v in ((0, 0), (9, 3), (-9, -3), (127, -127), (-127, 127), (-1, 0), (0, -1)):
        w = pg.pack_vector(*v)
        assert 0 <= w < 2 ** 32 and pg.unpack_vector(w) == v == m.ScanPipe.unpack_gmc_vector(w)
    # the same bits as the first word of mt_gmc_info
    info = np.zeros(1, dtype=_abi.GMC_INFO_DTYPE)
    info["gx"], info["gy"] = -9, 3
    assert int(info.view(np.uint32)[0]) == pg.pack_vector(-9, 3)
