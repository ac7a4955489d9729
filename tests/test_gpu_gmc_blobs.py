"""GPU tier (`-m gpu`): the compensated blob scan — motion blobs on the residuals of each frame's dominant vector
(include/mtgpu_gmc_blobs.h, csrc/gmc_blobs_kernels.hip).

Expected values: numbers derived by hand in tests/gmc_blobs_inputs.py and tests/blobs_inputs.py; the model of
tests/gmc_blobs_inputs.py (pipe_gmc_inputs.estimate + blobs_model.blob_stats) where a case says so; the existing entry
points mtgpu_scan_blobs_device and mtgpu_scan_gmc_device for consequences A and B.  tests/test_gmc_blobs_host.py holds all
of them against each other without a GPU.  Every comparison is exact; outputs are pre-filled with junk: every element
must be written by the call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, blobs, synth, tune

import blobs_inputs as bi
import blobs_model as bm
import derived_cliff_inputs as dci
import derived_edge_inputs as dei
import gmc_blobs_inputs as gbi
import gmc_inputs as gi
import gmc_model as gm
import pipe_gmc_inputs as pgi
import zones_inputs as zi
from scan_checks import to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG, JUNK_BOX = -7, 9, 0x1234
OUTPUTS = ("flags", "centres", "blobs", "largest", "box", "info")
BLOB_OUTPUTS = OUTPUTS[:5]
COUNTS = ("centres", "blobs", "largest")
MS, Q8 = gbi.MS, gbi.Q8


# ------------------------------------------------------------------ device helpers

def soff_tensor(stream_off):
    import torch
    return torch.from_numpy(np.asarray(stream_off).astype(np.int64)).cuda()


def keep_tensor(keeps):
    import torch
    return torch.from_numpy(zi.pack_keeps(keeps).view(np.int64).copy()).cuda()


def junk_outputs(n, want=OUTPUTS):
    import torch
    out = {}
    for k in want:
        if k == "flags":
            out[k] = torch.full((n,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
        elif k == "box":
            out[k] = torch.full((n, 4), JUNK_BOX, dtype=torch.int16, device="cuda")
        elif k == "info":
            out[k] = torch.full((n, 5), JUNK, dtype=torch.int32, device="cuda")
        else:
            out[k] = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    return out


def to_host(res):
    """{name: numpy array}: counts as uint32, box as uint16 [F, 4], info as int64 [F, 7] in the order of gbi.INFO_FIELDS."""
    out = {}
    for k, t in res.items():
        if t is None:
            continue
        a = t.cpu().numpy()
        if k == "flags":
            out[k] = a
        elif k == "box":
            out[k] = a.view(np.uint16)
        elif k == "info":
            out[k] = gbi.info_rows(np.ascontiguousarray(a).reshape(-1).view(_abi.GMC_INFO_DTYPE)) if a.size else np.zeros((0, 7), dtype=np.int64)
        else:
            out[k] = a.view(np.uint32)
    return out


def device_scan(s, d_rec, d_off, d_sd, compact, ms=MS, q8=Q8, min_blob=1, d_soff=None, d_keep=None, want=OUTPUTS, stream=None):
    """Through mtgpu_scan_gmc_blobs_device into junk-filled outputs -> {name: numpy array} on the host."""
    import torch
    out = junk_outputs(d_off.numel() - 1, want)
    torch.cuda.synchronize()
    res = s.scan_gmc_blobs_device(d_rec, d_off, d_sd, ms, q8, min_blob, d_soff, d_keep, compact=compact, want=want, out=out, stream=stream)
    torch.cuda.synchronize()
    return to_host(res)


def both_layouts(s, mv, off, sd, what, soff=None, keeps=None, **kw):
    """Both record layouts through the device entry point; yields (label, outputs)."""
    d_soff = soff_tensor(soff) if keeps is not None else None
    d_keep = keep_tensor(keeps) if keeps is not None else None
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        yield f"{what}, {'compact' if compact else '40-byte'}", device_scan(s, d_rec, d_off, d_sd, compact, d_soff=d_soff, d_keep=d_keep, **kw)


def assert_blobs(got, want, what, p=None, min_blob=1):
    """got: the call's outputs; want: {"centres", "blobs", "largest": per frame, "box": [F] of 4} — hand lists, the model's
    arrays or another entry point's outputs.  Exact; flags, where p is given, by the header's rule on the expected counts."""
    for k in COUNTS:
        g, w = got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)
        bad = np.flatnonzero(g != w) if g.shape == w.shape else np.arange(1)
        assert g.shape == w.shape and bad.size == 0, (f"{what}: {k} of {bad.size} of {w.size} frames differ, first {bad[:8].tolist()}: "
                                                      f"want {w[bad[:8]].tolist()} got {g[bad[:8]].tolist()}")
    gb, wb = got["box"].astype(np.int64).reshape(-1, 4), np.asarray(want["box"]).astype(np.int64).reshape(-1, 4)
    bad = np.flatnonzero((gb != wb).any(axis=1))
    assert bad.size == 0, f"{what}: boxes of frames {bad[:8].tolist()} differ: want {wb[bad[:8]].tolist()} got {gb[bad[:8]].tolist()}"
    if p is not None:
        wf = bm.flags_np(p, want["centres"], want["largest"], min_blob)
        assert got["flags"].tolist() == wf.tolist(), (what, "flags", got["flags"].tolist(), wf.tolist())


def assert_info(got, want_rows, what):
    g, w = np.asarray(got["info"]).astype(np.int64).reshape(-1, 7), np.asarray(want_rows).astype(np.int64).reshape(-1, 7)
    bad = np.flatnonzero((g != w).any(axis=1)) if g.shape == w.shape else np.arange(1)
    assert g.shape == w.shape and bad.size == 0, (f"{what}: info of frames {bad[:8].tolist()} differs ({gbi.INFO_FIELDS}): "
                                                  f"want {w[bad[:4]].tolist()} got {g[bad[:4]].tolist()}")


def hand_dict(rows):
    return bi.hand_of(rows)


# ------------------------------------------------------------------ 1. the rule bites

def test_the_rule_bites(gpu_scanner_factory):
    """The hand frames of gbi.bite_frames() (their numbers are re-derived in that docstring): four isolated pairs (P4) and
    one object of eight cells (O8) inside a pan of (9, 3).  The compensated blob scan tells them apart at min_blob_cells
    8; mtgpu_scan_gmc_device gives 8 centres for both; mtgpu_scan_blobs_device sees one blob of 2360 cells in both.  With
    a still overlay: five blobs without a mask, P4's values under a keep plane that clears it.  With the overlay in the
    majority (case D of pipe_gmc_inputs): nothing compensated without the mask, the pan goes with it (the model)."""
    p = pgi.params()
    s = gpu_scanner_factory(p)
    mv, off, sd = gbi.bite_batch(["P4", "O8"])
    want = hand_dict([gbi.BITE_HAND[0][3], gbi.BITE_HAND[1][3]])
    for label, got in both_layouts(s, mv, off, sd, "P4 / O8", min_blob=8):
        assert_blobs(got, want, label, p, 8)
        assert got["flags"].tolist() == [0, 1], label
        assert_info(got, [gbi.BITE_INFO, gbi.BITE_INFO], label)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        _, ce, _ = s.scan_gmc_device(d_rec, d_off, d_sd, MS, Q8, compact=compact)
        assert ce.cpu().numpy().view(np.uint32).tolist() == [8, 8]            # the compensated centre scan cannot tell them apart
        plain = s.scan_blobs_device(d_rec, d_off, d_sd, 8, compact=compact)
        c, b, g, box = gbi.BITE_PLAIN
        assert [plain[k].cpu().numpy().view(np.uint32).tolist() for k in COUNTS] == [[c, c], [b, b], [g, g]]
        assert plain["box"].cpu().numpy().view(np.uint16).tolist() == [list(box)] * 2 and plain["flags"].tolist() == [1, 1]
    # the overlay, without and with the keep plane that clears it
    mv, off, sd = gbi.bite_batch(["P4+overlay"])
    for name, _, keep, stats, info in gbi.BITE_HAND[2:]:
        keeps = None if keep is None else gbi.BITE_KEEPS[keep][None]
        for label, got in both_layouts(s, mv, off, sd, name, soff=[0, 1], keeps=keeps):
            assert_blobs(got, hand_dict([stats]), label, p)
            assert_info(got, [info], label)
    # the overlay in the majority
    mv, off, sd = gbi.bite_batch(["D"])
    for keeps in (None, pgi.KEEP_D[None]):
        want = gbi.model_batch(p, mv, off, sd, MS, Q8, np.array([0, 1]) if keeps is not None else None, keeps)
        assert tuple(want["info"][0][:2]) == ((0, 0) if keeps is None else (9, 3))
        assert int(want["centres"][0]) == (40 if keeps is None else 0)
        for label, got in both_layouts(s, mv, off, sd, "case D", soff=[0, 1], keeps=keeps):
            assert_blobs(got, want, label, p)
            assert_info(got, want["info"], label)


# ------------------------------------------------------------------ 2. the labelling under compensation

@pytest.mark.parametrize("name", list(gbi.REUSED))
def test_labelling_under_compensation(gpu_scanner_factory, name):
    """The pan embedding of a case of tests/blobs_inputs.py: by consequence C all five blob outputs equal the case's hand
    values; info from the model (the pan on both axes).  40-byte records with junk padding, and compact records."""
    c, e, plain = gbi.reused_case(name)
    s = gpu_scanner_factory(c.p)
    for emb, soff, keeps, hand in ((e, c.soff, c.keeps, c.hand), (plain, None, None, None)):
        if emb is None:
            continue
        if hand is None:
            hand = {k: [v[0]] * len(v) for k, v in c.hand.items()}
        info = gbi.model_batch(c.p, emb.mv, emb.off, c.sd, MS, Q8, soff, keeps)["info"]
        assert (info[np.flatnonzero(zi.has_side_data(c.off, c.sd))][:, :2] == emb.pan).all()
        for label, got in both_layouts(s, emb.mv, emb.off, c.sd, f"{name} under {emb.pan}", soff=soff, keeps=keeps):
            assert_blobs(got, hand, label, c.p)
            assert_info(got, info, label)


# ------------------------------------------------------------------ 3. consequences A and B

@pytest.mark.parametrize("i", gbi.RANDOM, ids=["%dx%d-mask%g-vn%d" % c for c in zi.RANDOM_CASES])
def test_consequences_a_and_b_on_random_batches(gpu_scanner_factory, i):
    """A: max_shift 0 == mtgpu_scan_blobs_device, all five outputs, with and without masks, min_blob_cells 1 and 3.
    B: without a mask centres and info == mtgpu_scan_gmc_device, and flags at min_blob_cells <= 1.  The rest == the model."""
    p, mv, off, sd, soff, keeps = zi.random_case(i)
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        lay = "compact" if compact else "40-byte"
        for masked in (False, True):
            d_soff, d_keep = (soff_tensor(soff), keep_tensor(keeps)) if masked else (None, None)
            for mb in (1, 3):
                ref = s.scan_blobs_device(d_rec, d_off, d_sd, mb, d_soff, d_keep, compact=compact)
                got = device_scan(s, d_rec, d_off, d_sd, compact, 0, Q8, mb, d_soff, d_keep)
                ref = {k: (v.cpu().numpy() if k == "flags" else v.cpu().numpy().view(np.uint16 if k == "box" else np.uint32)) for k, v in ref.items()}
                assert_blobs(got, ref, f"A: random {i}, {lay}, masks {masked}, min_blob {mb}")
                assert got["flags"].tolist() == ref["flags"].tolist()
                assert not got["info"][:, :4].any()
            want = gbi.model_batch(p, mv, off, sd, MS, 64, soff if masked else None, keeps if masked else None)
            got = device_scan(s, d_rec, d_off, d_sd, compact, MS, 64, 2, d_soff, d_keep)
            assert_blobs(got, want, f"model: random {i}, {lay}, masks {masked}", p, 2)
            assert_info(got, want["info"], f"model: random {i}, {lay}, masks {masked}")
        fl, ce, info = s.scan_gmc_device(d_rec, d_off, d_sd, MS, 64, compact=compact)
        for mb in (0, 1):
            got = device_scan(s, d_rec, d_off, d_sd, compact, MS, 64, mb)
            assert got["centres"].tolist() == ce.cpu().numpy().view(np.uint32).tolist(), f"B: random {i}, {lay}"
            assert got["flags"].tolist() == fl.cpu().numpy().tolist(), f"B: random {i}, {lay}"
            assert_info(got, gbi.info_rows(info.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)), f"B: random {i}, {lay}")


@pytest.mark.parametrize("vn", [0, 1])
def test_consequences_a_and_b_at_vn_0_and_1(gpu_scanner_factory, vn):
    """gmc_inputs.pan_batch() (record counts around the streamers' head, step and tail; random pans) at vectors_needed 0
    and 1: max_shift 0 against the blob scan, the default against the compensated centre scan and the model."""
    mv, off, sd, _, _ = gi.pan_batch()
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=vn, clusters_needed=1)
    s = gpu_scanner_factory(p)
    want = gbi.model_batch(p, mv, off, sd, gi.PAN_MAX_SHIFT, 128)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        ref = s.scan_blobs_device(d_rec, d_off, d_sd, 2, compact=compact)
        got = device_scan(s, d_rec, d_off, d_sd, compact, 0, 128, 2)
        ref = {k: (v.cpu().numpy() if k == "flags" else v.cpu().numpy().view(np.uint16 if k == "box" else np.uint32)) for k, v in ref.items()}
        assert_blobs(got, ref, f"A: vn {vn}")
        assert got["flags"].tolist() == ref["flags"].tolist()
        fl, ce, info = s.scan_gmc_device(d_rec, d_off, d_sd, gi.PAN_MAX_SHIFT, 128, compact=compact)
        got = device_scan(s, d_rec, d_off, d_sd, compact, gi.PAN_MAX_SHIFT, 128, 1)
        assert got["centres"].tolist() == ce.cpu().numpy().view(np.uint32).tolist() and got["flags"].tolist() == fl.cpu().numpy().tolist()
        assert_info(got, gbi.info_rows(info.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)), f"B: vn {vn}")
        assert_blobs(got, want, f"model: vn {vn}", p)


# ------------------------------------------------------------------ 4. per-stream masks

def test_per_stream_masks(gpu_scanner_factory):
    """Three streams, two planes: the same P4 + overlay frame reads 5 blobs in stream 0 (all ones) and P4's 4 in stream 1
    (the overlay cleared); frames behind stream_off[n_streams] read the no-blob answer and a zero info.  Consequence D:
    one stream, one plane against pipe_gmc_inputs.model."""
    p, mv, off, sd, soff, keeps = gbi.streams_case()
    s = gpu_scanner_factory(p)
    want = gbi.model_batch(p, mv, off, sd, MS, Q8, soff, keeps)
    for f, hand in enumerate(gbi.STREAMS_HAND):
        if hand is not None:
            assert (int(want["centres"][f]), int(want["blobs"][f]), int(want["largest"][f]), tuple(want["box"][f].tolist())) == hand, f
    assert not want["info"][[3, 5, 6]].any() and tuple(want["info"][0]) == (9, 3, 9, 3, 4860, 4784, 4800) and want["info"][2][4] == 4800
    for label, got in both_layouts(s, mv, off, sd, "three streams", soff=soff, keeps=keeps, min_blob=3):
        assert_blobs(got, want, label, p, 3)
        assert_info(got, want["info"], label)
        assert got["blobs"][0] == 5 and got["blobs"][2] == 4
    # D: one stream, one plane, the shapes of the compensated pipe's tests
    p, frames, keep = pgi.shapes_case()
    b = m.FrameBatch.from_frames(list(frames))
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE)
    off = np.ascontiguousarray(b.frame_off, dtype=np.uint64)
    sd = np.ascontiguousarray(b.has_sd, dtype=np.uint8)
    _, ce, ve = pgi.model(p, frames, MS, Q8, keep)
    for label, got in both_layouts(s, mv, off, sd, "D", soff=[0, len(frames)], keeps=keep[None]):
        assert got["centres"].tolist() == ce, label
        assert [pgi.pack_vector(r[0], r[1]) for r in got["info"]] == ve, label


# ------------------------------------------------------------------ 5. plumbing

def test_batch_plumbing(gpu_scanner_factory):
    """has_sd NULL; a frame with side data and no record; frames without side data that own records; the host entry on a
    window (frame_off[0] > 0); every single-output call leaves the other five untouched; guard elements around every
    output; n_frames == 0; a non-default stream."""
    import torch
    c, e = gbi.plumbing_case()
    assert e is not None
    p = c.p
    s = gpu_scanner_factory(p)
    hand = c.hand["plain"]
    info = gbi.model_batch(p, e.mv, e.off, c.sd, MS, Q8)["info"]
    for label, got in both_layouts(s, e.mv, e.off, c.sd, "plumbing"):
        assert_blobs(got, hand, label, p)
        assert_info(got, info, label)
    d_rec, d_off, d_sd = to_device(e.mv, e.off, c.sd, False)
    F = len(c.sd)
    # has_sd == NULL: side data iff records — frame 2 (the ring; has_sd was 0, so it got no fillers, only the shifted src) is
    # scanned now: every record of it moves by (5, 0) + (9, 3), which is its mode, and nothing is left; frame 3 owns nothing
    want = gbi.model_batch(p, e.mv, e.off, None, MS, Q8)
    got = device_scan(s, d_rec, d_off, None, False)
    assert_blobs(got, want, "has_sd NULL", p)
    assert_info(got, want["info"], "has_sd NULL")
    assert tuple(want["info"][2][:2]) == (5 + e.pan[0], e.pan[1]) == (14, 3)
    assert int(want["centres"][2]) == 0 and not want["info"][3].any()
    # every single-output call: the five others NULL and untouched; the output itself inside guard elements
    full = device_scan(s, d_rec, d_off, d_sd, False, min_blob=4)
    lib = m.load_library()
    for name in OUTPUTS:
        one = device_scan(s, d_rec, d_off, d_sd, False, min_blob=4, want=(name,))
        assert list(one) == [name] and np.array_equal(one[name], full[name]), name
        junk = junk_outputs(F + 2)                                           # one guard element in front and one behind
        step = {"flags": 1, "box": 8, "info": 20}.get(name, 4)
        ptrs = [junk[k].data_ptr() + step if k == name else None for k in OUTPUTS]
        torch.cuda.synchronize()
        rc = lib.mtgpu_scan_gmc_blobs_device(s._ctx, d_rec.data_ptr(), 40, len(e.mv), d_off.data_ptr(), d_sd.data_ptr(), F, None, 0, None,
                                             MS, Q8, 4, *ptrs, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.mtgpu_last_error()
        got, fresh = to_host(junk), to_host(junk_outputs(F + 2))
        assert np.array_equal(got[name][1:F + 1], full[name]), name
        assert np.array_equal(got[name][[0, F + 1]], fresh[name][[0, F + 1]]), (name, "guards")
        for other in OUTPUTS:
            if other != name:
                assert np.array_equal(got[other], fresh[other]), (name, "touched", other)
    # a non-default stream
    st = torch.cuda.Stream()
    got = device_scan(s, d_rec, d_off, d_sd, False, stream=st.cuda_stream)
    st.synchronize()
    assert_blobs(got, hand, "non-default stream", p)
    # n_frames == 0: MT_OK, nothing written, through both entry points
    empty = to_device(e.mv[:0], e.off[:1], c.sd[:0], False)
    assert all(v.size == 0 for v in device_scan(s, *empty, False).values())
    one = junk_outputs(1)
    rc = lib.mtgpu_scan_gmc_blobs_device(s._ctx, None, 40, 0, d_off.data_ptr(), None, 0, None, 0, None, MS, Q8, 1,
                                         *(one[k].data_ptr() for k in OUTPUTS), None)
    torch.cuda.synchronize()
    assert rc == 0 and one["flags"].item() == JUNK_FLAG and one["centres"].item() == JUNK and one["info"][0, 0].item() == JUNK
    r = s.scan_gmc_blobs(m.FrameBatch(e.mv[:0], e.off[:1], None, c.sd[:0]))
    assert all(len(v) == 0 for v in r.values())
    # the host entry point, whole and on a window that does not start at record 0
    for lo, hi in ((0, F), (4, 7)):
        r = s.scan_gmc_blobs(m.FrameBatch(e.mv, e.off[lo:hi + 1], None, c.sd[lo:hi]), MS, Q8, 1)
        r["box"] = r["box"].view(np.uint16).reshape(-1, 4)
        assert int(e.off[4]) > 0
        assert_blobs(r, {k: v[lo:hi] for k, v in hand.items()}, f"host entry {lo}:{hi}", p)
        assert_info({"info": gbi.info_rows(r["info"])}, info[lo:hi], f"host entry {lo}:{hi}")
    with pytest.raises(ValueError):
        s.scan_gmc_blobs(m.FrameBatch(e.mv, e.off, None, c.sd), MS, Q8, 1, [0, F], None)
    # a frame with side data and no record, alone; an empty analysed range (vertical_mask 0.5)
    got = device_scan(s, *to_device(e.mv[:0], np.zeros(2, dtype=np.uint64), np.ones(1, dtype=np.uint8), False), False)
    assert [got[k].tolist() for k in COUNTS] == [[0], [0], [0]] and got["box"].tolist() == [[0xFFFF] * 4] and not got["info"].any()
    pe = m.ScanParams.from_config(1920, 1080, vertical_mask=0.5)
    se = gpu_scanner_factory(pe)
    mv, off, sd = gbi.bite_batch(["P4", "O8"])
    keeps = np.ones((1, pe.grid_h, pe.grid_w), dtype=bool)
    for k in (None, keeps):
        for label, got in both_layouts(se, mv, off, sd, "empty analysed range", soff=[0, 2], keeps=k):
            assert [got[n].tolist() for n in COUNTS] == [[0, 0]] * 3 and not got["info"].any() and got["flags"].tolist() == [0, 0], label


def test_validation_errors_leave_the_outputs_untouched(gpu_scanner_factory):
    import torch
    p = pgi.params()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    mv, off, sd = gbi.bite_batch(["P4", "O8"])
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    d_soff, d_keep = soff_tensor([0, 2]), keep_tensor(pgi.ONES[None])
    F = 2

    def run(rec_bytes=40, ms=MS, q8=Q8, soff=None, ns=0, keep=None, ctx=None, over=None, off_ptr=None):
        junk = junk_outputs(F)
        ptrs = {k: junk[k].data_ptr() for k in OUTPUTS}
        ptrs.update(over or {})
        torch.cuda.synchronize()
        rc = lib.mtgpu_scan_gmc_blobs_device((ctx or s)._ctx, d_rec.data_ptr(), rec_bytes, len(mv), d_off.data_ptr() if off_ptr is None else off_ptr,
                                             d_sd.data_ptr(), F, soff, ns, keep, ms, q8, 1, *(ptrs[k] for k in OUTPUTS), None)
        torch.cuda.synchronize()
        msg = lib.mtgpu_last_error().decode()
        fresh = junk_outputs(F)
        clean = all(torch.equal(junk[k], fresh[k]) for k in OUTPUTS)
        return rc, msg, clean
    inv = _abi.MT_ERR_INVALID
    for kw, word in ((dict(rec_bytes=16), "rec_bytes"), (dict(ms=128), "max_shift"), (dict(ms=-1), "max_shift"), (dict(q8=257), "min_share_q8"),
                     (dict(keep=d_keep.data_ptr()), "d_stream_off is NULL"), (dict(keep=d_keep.data_ptr(), soff=d_soff.data_ptr()), "n_streams is 0"),
                     (dict(soff=d_soff.data_ptr()), "d_keep is NULL"), (dict(ns=1), "d_keep is NULL"),
                     (dict(off_ptr=d_off.data_ptr() + 4), "d_frame_off must be 8-byte aligned"),
                     (dict(over={"info": d_rec.data_ptr() + 2}), "d_info must be 4-byte aligned"),
                     (dict(over={"box": d_rec.data_ptr() + 1}), "d_box must be 2-byte aligned")):
        rc, msg, clean = run(**kw)
        assert rc == inv and word in msg and clean, (kw, msg)
    pinned = torch.full((F * 8,), JUNK, dtype=torch.int32).pin_memory()
    for name in OUTPUTS:
        rc, msg, clean = run(over={name: pinned.data_ptr()})
        assert rc == inv and ("d_" + name + " is not memory of device") in msg and clean, (name, msg)
        assert int((pinned != JUNK).sum()) == 0
    rc, msg, clean = run(keep=pinned.data_ptr(), soff=d_soff.data_ptr(), ns=1)
    assert rc == inv and "d_keep is not memory of device" in msg and clean
    # the row-banded grid: MT_ERR_UNSUPPORTED with the grid named, on both entry points
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, **gbi.FINE_KW))
    rc, msg, clean = run(ctx=big)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg and clean
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_gmc_blobs(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # the host entry's own: stream_off[n_streams] != n_frames
    with pytest.raises(m.MtgpuError) as ei:
        s.scan_gmc_blobs(m.FrameBatch(mv, off, None, sd), MS, Q8, 1, [0, 1], zi.pack_keeps(pgi.ONES[None]))
    assert ei.value.code == inv and "not n_frames" in str(ei.value)
    rc, msg, clean = run()
    assert rc == 0 and not clean


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    p = pgi.params()
    s = gpu_scanner_factory(p)
    mv, off, sd = gbi.bite_batch(["P4", "O8"])
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_scan(s, d_rec, d_off, d_sd, False, min_blob=8)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert got["flags"].tolist() == [0, 1]


def test_clear_kernels_second_trip(gpu_scanner_factory):
    """gmc_inputs.clear_batch(): 262 144 + 300 frames of which four have side data: gmc_blobs_clear_kernel (1024 x 256
    lanes) writes the elements from 262 144 on in a second trip of its loop.  The planted frames read the hand values of
    gmc_inputs (4 centres: the 2 x 2 object, one blob, box (3, 2, 4, 3); info (5, 0, 5, 0, 48, 44, 48)), every other frame
    0, an all-0xFFFF box and a zero info."""
    mv, off, sd, planted = gi.clear_batch()
    F, idx = gi.CLEAR_FRAMES, list(planted)
    thr, margin, _, ms, q8, info1, c1, _ = gi.HAND[gi.CLEAR_CASE]
    assert c1 == 4
    s = gpu_scanner_factory(gi.hand_params(thr, margin))
    want = {k: np.zeros(F, dtype=np.int64) for k in COUNTS}
    want["centres"][idx], want["blobs"][idx], want["largest"][idx] = 4, 1, 4
    want["box"] = np.full((F, 4), 0xFFFF, dtype=np.int64)
    want["box"][idx] = (3, 2, 4, 3)
    info = np.zeros((F, 7), dtype=np.int64)
    info[idx] = info1
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        got = device_scan(s, d_rec, d_off, d_sd, compact, ms, q8, 4)
        assert_blobs(got, want, f"{F} frames, compact {compact}")
        assert_info(got, info, f"{F} frames, compact {compact}")
        assert np.flatnonzero(got["flags"]).tolist() == idx


def test_support_and_pick_in_64_bits_under_an_all_ones_keep(gpu_scanner_factory):
    """gmc_inputs.HUGE (2^24 + 2 records in one frame) under an all-ones keep plane: the masked estimate's path.  At
    min_share_q8 256 x is unsupported and the two cells keep their residuals: 2 centres, one blob of 2, box (1, 1, 2, 1);
    at 255 the pan is applied and nothing is left."""
    import torch
    a, b, c = m.pack_records(dei.voters(gi.HUGE_TRIPLE, 4)).view(np.int64).tolist()
    d_rec = torch.empty(gi.HUGE_N, dtype=torch.int64, device="cuda")
    d_rec[0::2], d_rec[1::2] = a, b
    d_rec[-1] = c
    d_off = torch.tensor([0, gi.HUGE_N], dtype=torch.int64, device="cuda")
    d_sd = torch.ones(1, dtype=torch.uint8, device="cuda")
    s = gpu_scanner_factory(gi.hand_params(16.0, 0))
    d_soff, d_keep = soff_tensor([0, 1]), keep_tensor(np.ones((1, gi.GH, gi.GW), dtype=bool))
    for q8, (want_i, want_c) in gi.HUGE.items():
        got = device_scan(s, d_rec, d_off, d_sd, True, 16, q8, 2, d_soff, d_keep)
        assert_info(got, [want_i], f"2^24 + 2 records, min_share_q8 {q8}")
        stats = (2, 1, 2, (1, 1, 2, 1)) if want_c else (0, 0, 0, bm.NO_BOX)
        assert want_c == stats[0]
        assert_blobs(got, hand_dict([stats]), f"2^24 + 2 records, min_share_q8 {q8}")
        assert got["flags"].tolist() == [int(want_c >= 2)]


# ------------------------------------------------------------------ 6. limits

@pytest.mark.parametrize("name", ["tall-3", "tall-65", "wide-1", "wide-3"])
def test_last_grid_the_preview_accepts(gpu_scanner_factory, name):
    """The last grids mtgpu_gmc_blobs_preview accepts (bisection in gbi.limit_shapes), each with the 12-frame batch of
    derived_cliff_inputs under the pan embedding: centres of the planted frames by dci.hand_count, the rest by the model."""
    gw, gh, kind = gbi.limit_shapes()[name]
    p, (mv, off, sd, planted), e = gbi.limit_case(name)
    assert e is not None and m.gmc_blobs_preview(p)["lds_bytes"] == gbi.lds_by_hand(gw, gh) <= bi.MI355X_LDS
    want = gbi.model_batch(p, e.mv, e.off, sd, MS, Q8)
    s = gpu_scanner_factory(p)
    for label, got in both_layouts(s, e.mv, e.off, sd, f"limit {name} {gw}x{gh}"):
        for kind_ in ("E", "H", "VL", "VR"):
            for f in dci.frames_named(kind_):
                assert int(got["centres"][f]) == dci.hand_count(planted[kind_], gw, gh, 4.0, 2), (label, kind_)
        assert_blobs(got, want, label, p)
        assert_info(got, want["info"], label)


def test_row_banded_grid_is_unsupported(gpu_scanner_factory):
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, **gbi.FINE_KW))
    import torch
    off = torch.zeros(2, dtype=torch.int64, device="cuda")
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_gmc_blobs_device(torch.zeros(0, dtype=torch.uint8, device="cuda"), off, None)
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)


# ------------------------------------------------------------------ 7. consequence E

def test_largest_through_the_sweep_is_flags_through_the_merge(gpu_scanner_factory):
    """The sweep input of the blob tests under the pan embedding, clusters_needed 1, levels 1, 2, 4, 8:
    mtgpu_sweep_streams_device on `largest` == mtgpu_merge_streams_device on flags at min_blob_cells = L, segment for
    segment, bit patterns compared."""
    import torch
    p, mv, off, sd, pts, soff = bi.sweep_case()
    e = gbi.embed(p, mv, off, sd, (9, 3), seed=10)
    assert e is not None
    s = gpu_scanner_factory(p)
    CAP = 16
    d_rec, d_off, d_sd = to_device(e.mv, e.off, sd, True)
    d_pts, d_soff = torch.from_numpy(pts.copy()).cuda(), soff_tensor(soff)
    mps = [m.MergeParams(duration=48 / 25.0, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0) for _ in range(2)]
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    levels = list(bi.SWEEP_LEVELS)
    res = s.scan_gmc_blobs_device(d_rec, d_off, d_sd, MS, Q8, 1, compact=True)
    sseg, sres = s.sweep_streams_device(res["largest"], d_pts, d_soff, d_mp, levels, seg_cap=CAP)
    torch.cuda.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)        # noqa: E731
    kept = []
    for li, lv in enumerate(levels):
        fl = s.scan_gmc_blobs_device(d_rec, d_off, d_sd, MS, Q8, lv, compact=True, want=("flags",))["flags"]
        seg, r8 = s.merge_streams_device(fl, d_pts, d_soff, d_mp, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg.cpu().numpy())), lv
        assert np.array_equal(sres[li].cpu().numpy(), r8.cpu().numpy()), lv
        kept.append(int(fl.sum()))
    assert kept == [96, 96, 48, 24]


# ------------------------------------------------------------------ 8. the example and the command

def test_plain_c_gmc_blobs_example(tmp_path):
    """examples/gmc_blobs_example.c: the four pairs against the one object, three scans side by side (it checks its own
    numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "gmc_blobs_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "gmc_blobs_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "motion frames with a minimum of 8: blobs 2, gmc 2, gmc + blobs 1 of 2" in out.stdout
    assert "frame 1  blobs: 2360 centres in 1 blobs, largest 2360" in out.stdout and "8 centres in 1 blobs, largest 8 at (50, 25) .. (53, 26)" in out.stdout


def test_end_to_end_command(gpu_scanner_factory, tmp_path, capsys):
    """`python -m mvtrim_amd.blobs --gmc --json` on a synth.StreamSpec(shake=5) stream written as .mtmv, in a fresh child
    process: its rows equal the Python layer's (blobs.measure with the settings).  Without --gmc the command's output
    equals blobs.measure without settings — the same function, the flag off — and carries no gmc key."""
    F = 24
    spec = synth.StreamSpec(640, 368, 16, 1, fps=25.0, gop=10, seed=5, salt_p=0.0, oob_p=0.0, shake=5,
                            events=[synth.Event(8, 16, 10, 8, 4, 3, 9, 2)])
    frames = [synth.gen_frame(spec, f) for f in range(F)]
    path = str(tmp_path / "shaken.mtmv")
    m.mvfile.write_mtmv(path, 640, 368, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    batch, fpts, hdr = tune.load(path)
    p = m.ScanParams.from_config(640, 368, vectors_needed=1, clusters_needed=1)
    s = gpu_scanner_factory(p)
    mp = m.MergeParams(duration=F / 25.0, max_gap_sec=0.2, padding_sec=0.04, min_savings_pct=5.0)
    direct = blobs.measure(s, batch, fpts, [1, 2, 4, 8], mp, None, (16, 77))
    plain = blobs.measure(s, batch, fpts, [1, 2, 4, 8], mp)
    assert "vectors" in direct and "vectors" not in plain and "compensated_share" not in plain
    # the Python layer against the model: the largest residual blob per frame
    mv = np.ascontiguousarray(batch.mv, dtype=m.MV_DTYPE)
    want = gbi.model_batch(p, mv, batch.frame_off, batch.has_sd, 16, 77)
    assert direct["largest_blob"] == int(want["largest"].max()) and direct["centres"] == int(want["centres"].sum())
    assert [r["min_blob_cells"]["motion_frames"] for r in direct["levels"]] == [int((want["largest"] >= lv).sum()) for lv in (1, 2, 4, 8)]
    assert direct["levels"][3]["min_blob_cells"]["motion_frames"] < plain["levels"][3]["min_blob_cells"]["motion_frames"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [path, "--vectors-needed", "1", "--max-gap-sec", "0.2", "--padding-sec", "0.04", "--min-savings-pct", "5"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.blobs"] + args + ["--gmc", "--min-share", "0.3", "--json"], capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert (doc["max_shift"], doc["min_share_q8"]) == (16, 77)
    for k in ("levels", "blobs_per_frame", "largest_blob", "centres", "compensated_share", "vectors"):
        assert doc[k] == direct[k], k
    # without --gmc, in this process: JSON and table
    capsys.readouterr()
    assert blobs.main(args + ["--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert sorted(doc) == sorted(["file", "width", "height", "grid_w", "grid_h", "frames", "keep"] + list(plain))
    for k in plain:
        assert doc[k] == plain[k], k
    assert blobs.main(args + ["--gmc", "--min-share", "0.3"]) == 0
    text = capsys.readouterr().out
    assert "# gmc: max_shift 16, min_share 77/256;" in text and "most frequent:" in text and "MIN_BLOB_CELLS" in text
    assert blobs.main(args) == 0
    assert "gmc" not in capsys.readouterr().out
