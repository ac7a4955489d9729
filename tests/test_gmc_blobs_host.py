"""CPU tier: the compensated blob scan (include/mtgpu_gmc_blobs.h) exists at every layer — header, library, ctypes table,
Python methods, the `blobs --gmc` flags — and the inputs of tests/test_gpu_gmc_blobs.py are what they claim to be: the
model returns every hand-derived number, the pan embedding has its properties on every reused case, and the limit shapes
sit on the limit.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, blobs

import blobs_inputs as bi
import blobs_model as bm
import derived_cliff_inputs as dci
import gmc_blobs_inputs as gbi
import gmc_model as gm
import pipe_gmc_inputs as pgi
import zones_inputs as zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840
NEW_SYMBOLS = ["mtgpu_gmc_blobs_preview", "mtgpu_scan_frames_gmc_blobs", "mtgpu_scan_gmc_blobs_device"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_gmc_blobs.h")).read()


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_GMC_BLOBS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_GMC_BLOBS[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
    assert '#include "mtgpu_gmc_blobs.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert C.sizeof(_abi.GmcBlobsPlanC) == 24
    assert [f for f, _ in _abi.GmcBlobsPlanC._fields_] == ["lds_bytes", "workgroup", "keep_words_per_row", "keep_words_per_stream",
                                                           "hist_bins", "info_bytes"]
    # the header states the five consequences the GPU tests rest on, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("A. max_shift == 0 equals mtgpu_scan_blobs_device", "B. Without a mask, centres and info equal mtgpu_scan_gmc_device's",
                 "C. A frame's five blob outputs equal mtgpu_scan_blobs_device's", "D. With one stream and one plane",
                 "E. For a level L >= max(1, cn)", "still refuse the pair", "an all-0xFFFF box and an all-zero info"):
        assert text in flat, text
    # the parents point at it and still say the pipe refuses the pair
    for name in ("mtgpu_gmc.h", "mtgpu_blobs.h"):
        parent = " ".join(open(os.path.join(ROOT, "include", name)).read().replace("*", " ").split())
        assert "mtgpu_gmc_blobs.h" in parent and "refuse" in parent, name
    src = open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "gmc_blobs_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "amdgpu_waves_per_eu(8, 8)" in src
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"gmc_blobs_frames_kernel" in blob and b"gmc_blobs_clear_kernel" in blob


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_gmc_blobs_plan p;\n"
            "  mt_blob_box b = {0, 0, 0, 0};\n"
            "  mt_gmc_info i;\n"
            "  i.gx = i.gy = i.mode_x = i.mode_y = 0; i.n_in = i.n_x = i.n_y = 0;\n"
            "  return mtgpu_gmc_blobs_preview(0, 163840, &p)\n"
            "       + mtgpu_scan_gmc_blobs_device(c, 0, 40, 0, 0, 0, 0, 0, 0, 0, 16, 128, 1, 0, 0, 0, 0, &b, &i, 0)\n"
            "       + mtgpu_scan_frames_gmc_blobs(c, 0, 0, 0, 0, 0, 0, 0, 16, 128, 1, 0, 0, 0, 0, &b, &i)\n"
            "       + p.lds_bytes + p.workgroup + p.keep_words_per_row + p.keep_words_per_stream + p.hist_bins + p.info_bytes;\n}\n")
    for first in ("mtgpu.h", "mtgpu_gmc_blobs.h", "mtgpu_gmc.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/gmc_blobs_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "gmc_blobs_example.c")])


def test_package_exports_the_methods():
    for name in ("scan_gmc_blobs", "scan_gmc_blobs_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.gmc_blobs_preview) and "gmc_blobs_preview" in m.__all__


# ------------------------------------------------------------------ preview

def preview(params, lds=MI355X_LDS):
    p = _abi.GmcBlobsPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_gmc_blobs_preview(C.byref(c), lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def lds_formula(gw, R):
    """Written out once more, from the table of csrc/gmc_blobs_kernels.h, region by region."""
    W = (gw + 63) // 64
    tile = 4 * (((R + 2) * gw + 3) & ~3)
    keep, amask, hist, res, total = R * W * 8, (R + 2) * W * 8, 2 * 256 * 4, 8 * 4, 8 * 4
    return tile + keep + amask + hist + res + total


def test_preview_sizes_the_launch():
    for (w, h, kw), (gw, gh, R) in [((1920, 1080, {}), (120, 68, 62)), ((3840, 2160, {}), (240, 135, 123)),
                                     ((3840, 2160, dict(vertical_mask=0.0)), (240, 135, 135)), ((1280, 720, {}), (80, 45, 41)),
                                     ((48, 48, dict(vertical_mask=0.0)), (3, 3, 3)), ((1920, 1080, dict(vertical_mask=0.5)), (120, 68, 1))]:
        params = m.ScanParams.from_config(w, h, **kw)
        assert (params.grid_w, params.grid_h) == (gw, gh) and max(1, gh - 2 * params.vertical_margin) == R
        rc, p, msg = preview(params)
        assert rc == _abi.MT_OK, msg
        W = (gw + 63) // 64
        assert (p.workgroup, p.keep_words_per_row, p.keep_words_per_stream, p.hist_bins, p.info_bytes) == (1024, W, W * gh, 256, 20)
        assert p.lds_bytes == lds_formula(gw, R) == gbi.lds_by_hand(gw, R) <= MI355X_LDS
        # the blob scan's layout plus the histograms and the result words, and the grid alone decides
        assert p.lds_bytes == m.blobs_preview(params)["lds_bytes"] + 2 * 256 * 4 + 32
        assert m.gmc_blobs_preview(params)["lds_bytes"] == p.lds_bytes
    # two 1080p workgroups per CU are limited by lanes, not LDS; 4K sits alone on its CU
    assert 2 * preview(m.ScanParams.from_config(1920, 1080))[1].lds_bytes <= MI355X_LDS
    assert 2 * preview(m.ScanParams.from_config(3840, 2160))[1].lds_bytes > MI355X_LDS
    # the row-banded grids have no form and are named; nor has 1080p on a device with 32 KB
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, **gbi.FINE_KW))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    rc, _, msg = preview(m.ScanParams.from_config(1920, 1080), 32768)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg
    with pytest.raises(m.MtgpuError) as ei:
        m.gmc_blobs_preview(m.ScanParams.from_config(3840, 2160, **gbi.FINE_KW))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
    # invalid
    lib = m.load_library()
    c = m.ScanParams.from_config(1920, 1080).to_c()
    out = _abi.GmcBlobsPlanC()
    assert lib.mtgpu_gmc_blobs_preview(C.byref(c), 163840, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_gmc_blobs_preview(None, 163840, C.byref(out)) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_gmc_blobs_preview(C.byref(c), 512, C.byref(out)) == _abi.MT_ERR_INVALID


def test_limit_shapes_sit_on_the_limit():
    """One more row (tall) or column (wide) is MT_ERR_UNSUPPORTED, the shape itself fits by the hand formula, and the blob
    scan's own limit shapes — which have 2080 bytes more to spend — are rejected."""
    shapes = gbi.limit_shapes()
    assert sorted(shapes) == ["tall-3", "tall-65", "wide-1", "wide-3"]
    for name, (gw, gh, kind) in shapes.items():
        p = dci.grid_params(gw, gh)
        assert gbi.preview_or_none(p)["lds_bytes"] == gbi.lds_by_hand(gw, gh) <= MI355X_LDS, name
        gw1, gh1 = dci.one_more(gw, gh, kind)
        assert gbi.lds_by_hand(gw1, gh1) > MI355X_LDS, name
        rc, _, msg = preview(dci.grid_params(gw1, gh1))
        assert rc == _abi.MT_ERR_UNSUPPORTED and f"{gw1}x{gh1}" in msg, (name, msg)
        # several trips of the workgroup over the keep words (tall) / many words per row (wide)
        W = (gw + 63) // 64
        assert (gh * W > 1024) if kind == "tall" else (W > 64), name
    for kind, (gw, gh) in bi.limit_shapes().items():
        assert gbi.preview_or_none(bi.limit_params(gw, gh)) is None, kind
    # no null call reaches a device
    lib = m.load_library()
    assert lib.mtgpu_scan_gmc_blobs_device(None, None, 40, 0, None, None, 0, None, 0, None, 16, 128, 1, *([None] * 6), None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_scan_frames_gmc_blobs(None, None, None, None, 0, None, 0, None, 16, 128, 1, *([None] * 6)) == _abi.MT_ERR_INVALID


def test_argument_errors_need_no_device():
    """What the arguments alone decide is answered before the context is looked at (ctx NULL here), with the argument
    named."""
    lib = m.load_library()
    one = np.zeros(8, dtype=np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    out = [vp(one)] + [None] * 5

    def dev(rec_bytes=40, ms=16, q8=128, soff=None, ns=0, keep=None, outs=out, off=vp(one)):
        rc = lib.mtgpu_scan_gmc_blobs_device(None, None, rec_bytes, 0, off, None, 1, soff, ns, keep, ms, q8, 1, *outs, None)
        return rc, lib.mtgpu_last_error().decode()
    for kw, word in ((dict(rec_bytes=16), "rec_bytes"), (dict(ms=128), "max_shift"), (dict(ms=-1), "max_shift"), (dict(q8=257), "min_share_q8"),
                     (dict(q8=-1), "min_share_q8"), (dict(outs=[None] * 6), "all NULL"), (dict(off=None), "d_frame_off"),
                     (dict(keep=vp(one)), "d_stream_off"), (dict(keep=vp(one), soff=vp(one)), "n_streams"),
                     (dict(soff=vp(one)), "d_keep"), (dict(ns=2), "n_streams"), ({}, "ctx")):
        rc, msg = dev(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)
    odd = C.c_void_p(one.ctypes.data + 1)
    for i, word in enumerate(("", "d_centres", "d_blobs", "d_largest", "d_box", "d_info")):
        if word:
            rc, msg = dev(outs=[odd if j == i else None for j in range(6)])
            assert rc == _abi.MT_ERR_INVALID and word in msg, msg

    def host(ms=16, q8=128, off=one, soff=None, ns=0, keep=None, outs=out, n=1):
        rc = lib.mtgpu_scan_frames_gmc_blobs(None, None, vp(off) if off is not None else None, None, n, vp(soff) if soff is not None else None,
                                             ns, vp(keep) if keep is not None else None, ms, q8, 1, *outs)
        return rc, lib.mtgpu_last_error().decode()
    down = np.array([5, 3], dtype=np.uint64)
    for kw, word in ((dict(ms=200), "max_shift"), (dict(q8=300), "min_share_q8"), (dict(outs=[None] * 6), "all NULL"), (dict(off=None), "frame_off"),
                     (dict(off=down), "not monotonic"), (dict(keep=one), "stream_off"), (dict(soff=one), "keep is NULL"),
                     (dict(keep=one, soff=down, ns=1), "stream_off not monotonic"),
                     (dict(keep=one, soff=np.array([0, 2], dtype=np.uint64), ns=1), "not n_frames"), ({}, "ctx")):
        rc, msg = host(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)


# ------------------------------------------------------------------ the model against the hand values

def test_model_returns_the_hand_values_of_the_bite_frames():
    p = pgi.params()
    fr = gbi.bite_frames()
    for name, frame, keep, stats, info in gbi.BITE_HAND:
        got_stats, got_info = gbi.frame_model(p, fr[frame], gbi.MS, gbi.Q8, gbi.BITE_KEEPS[keep])
        assert got_stats == stats and got_info == info, (name, got_stats, got_info)
    # the two scans that exist cannot tell P4 from O8: the compensated centre count is 8 for both ...
    for name in ("P4", "O8"):
        assert gm.gmc_frame(p, fr[name], gbi.MS, gbi.Q8)[0] == 8
        # ... and the plain blob scan sees the panned region as one blob
        assert bm.frame_stats(p, fr[name]) == gbi.BITE_PLAIN
    # min_blob_cells 8 tells them apart
    for name, want in (("P4", 0), ("O8", 1)):
        (c, _, g, _), _ = gbi.frame_model(p, fr[name], gbi.MS, gbi.Q8)
        assert int(bm.flags_np(p, [c], [g], 8)[0]) == want
    # the overlay in the majority (case D): nothing is compensated without the mask, the pan goes with it
    (_, info_plain), (stats_mask, info_mask) = gbi.frame_model(p, fr["D"], gbi.MS, gbi.Q8), gbi.frame_model(p, fr["D"], gbi.MS, gbi.Q8, pgi.KEEP_D)
    assert info_plain[:2] == (0, 0) and info_mask[:2] == (9, 3) and stats_mask == (0, 0, 0, bm.NO_BOX)
    assert gbi.frame_model(p, fr["D"], gbi.MS, gbi.Q8)[0][0] == 40


def test_model_is_its_parents():
    """max_shift 0 is blobs_model; without a mask centres and info are gmc_model's; with one plane centres and the vector
    are pipe_gmc_inputs.model's — on the random batches of the zones tests."""
    for i in (0, 3, 5):
        p, mv, off, sd, soff, keeps = zi.random_case(i)
        for masked in (False, True):
            kw = dict(soff=soff, keeps=keeps) if masked else {}
            got = gbi.model_batch(p, mv, off, sd, 0, 128, **kw)
            want = bm.model_batch(p, mv, off, sd, soff if masked else None, keeps if masked else None)
            for k in ("centres", "blobs", "largest", "box"):
                assert np.array_equal(got[k], want[k]), (i, masked, k)
        got = gbi.model_batch(p, mv, off, sd, 16, 64)
        _, centres, info = gm.gmc_batch(p, mv, off, sd, 16, 64)
        assert np.array_equal(got["centres"], centres) and np.array_equal(got["info"], gbi.info_rows(info))
    p, frames, keep = pgi.shapes_case()
    b = m.FrameBatch.from_frames(list(frames))
    got = gbi.model_batch(p, b.mv, b.frame_off, b.has_sd, 16, 128, np.array([0, len(frames)], dtype=np.uint64), keep[None])
    _, ce, ve = pgi.model(p, frames, 16, 128, keep)
    assert got["centres"].tolist() == ce
    assert [pgi.pack_vector(r[0], r[1]) for r in got["info"]] == ve


# ------------------------------------------------------------------ the pan embedding

@pytest.mark.parametrize("name", list(gbi.REUSED))
def test_embedding_has_its_properties(name):
    """No case is left out: the embedding returns a batch for every reused case.  Then: no src left int16 (the arrays are
    int16: the check is that subtracting the pan gives the original back), strictly more fillers than own records in
    every frame with side data, both modes are the pan with a share above one half, and the model of the embedded batch
    gives the case's hand values."""
    c, e, plain = gbi.reused_case(name)
    assert e is not None, name
    for emb, soff, keeps in ((e, c.soff, c.keeps), (plain, None, None)):
        if emb is None:
            continue
        a, b = emb.pan
        assert (abs(a), abs(b)) == tuple(abs(v) for v in gbi.REUSED[name][1]) and max(abs(a), abs(b)) <= gbi.MS
        own = np.diff(c.off.astype(np.int64))
        has = zi.has_side_data(c.off, c.sd)
        assert all(f > o for f, o, h in zip(emb.fillers, own, has) if h) and all(f == 0 for f, h in zip(emb.fillers, has) if not h)
        assert np.array_equal(np.diff(emb.off.astype(np.int64)), own + np.array(emb.fillers))
        dx, dy = gm.displacements(emb.mv)
        assert np.sort(dx).tolist() == np.sort(np.concatenate([gm.displacements(c.mv)[0] + a, np.full(sum(emb.fillers), a)])).tolist()
        want = gbi.model_batch(c.p, emb.mv, emb.off, c.sd, gbi.MS, gbi.Q8, soff, keeps)
        for f in np.flatnonzero(has):
            gx, gy, mx, my, n_in, nx, ny = want["info"][f]
            assert (gx, gy, mx, my) == (a, b, a, b) and 2 * nx > n_in and 2 * ny > n_in and nx >= emb.fillers[f], (name, f)
        # the seam cases without their masks: every frame reads the full-mask stream's values (blobs_inputs.seam_case)
        hand = c.hand if emb is e else {k: [v[0]] * len(v) for k, v in c.hand.items()}
        for k in ("centres", "blobs", "largest"):
            assert want[k].tolist() == list(hand[k]), (name, k)
        assert [tuple(r) for r in want["box"].tolist()] == [tuple(b_) for b_ in hand["box"]], name


def test_limit_batches_embed_and_carry_centres():
    for name, (gw, gh, kind) in gbi.limit_shapes().items():
        p, (mv, off, sd, planted), e = gbi.limit_case(name)
        assert e is not None and e.pan == gbi.LIMIT_PAN, name
        want = gbi.model_batch(p, e.mv, e.off, sd, gbi.MS, gbi.Q8)
        for kind_, idx in (("E", dci.frames_named("E")), ("H", dci.frames_named("H"))):
            for f in idx:
                assert int(want["centres"][f]) == dci.hand_count(planted[kind_], gw, gh, 4.0, 2), (name, kind_)
        assert int(want["centres"].sum()) > 0 and (want["info"][np.flatnonzero(sd)][:, :2] == gbi.LIMIT_PAN).all(), name


# ------------------------------------------------------------------ the command's flags

def test_blobs_gmc_usage_errors(capsys):
    for args in (["x.mtmv", "--max-shift", "4"], ["x.mtmv", "--min-share", "0.5"], ["x.mtmv", "--gmc", "--max-shift", "128"],
                 ["x.mtmv", "--gmc", "--max-shift", "-1"], ["x.mtmv", "--gmc", "--min-share", "1.5"], ["x.mtmv", "--gmc", "--min-share", "-0.1"]):
        with pytest.raises(SystemExit) as ei:
            blobs.main(args)
        assert ei.value.code == 2, args
        assert "usage" in capsys.readouterr().err
    ns = blobs.parser().parse_args(["x.mtmv", "--gmc"])
    assert ns.gmc and ns.max_shift is None and ns.min_share is None
