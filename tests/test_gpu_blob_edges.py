"""GPU tier (`-m gpu`): the record-level edge cases of the scan's suite held against the streamers of
csrc/record_stream.h as the blob kernels instantiate them — blobs_frames_kernel in its resident and its pipe form
(csrc/blobs_kernels.hip), gmc_blobs_frames_kernel's three streaming call sites (the unmasked estimate, the masked
estimate that reads a keep word per record, the residual vote; csrc/gmc_blobs_kernels.hip) — and gmc_frames_kernel in its
resident and pipe form.  Each of them streams a frame's records twice or, for the blob scans, once per pass.

Inputs: tests/derived_edge_inputs.py as they are (edge_batch, unaligned_batch, big_frames); what is added lives in
tests/blob_edges_inputs.py, and tests/test_blob_edges_host.py holds every expected value without a GPU.  Every comparison
is `==` on integers, every output starts as junk, and both record layouts run wherever the entry point has them."""
import contextlib

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import blob_edges_inputs as bei
import blobs_model as bm
import derived_edge_inputs as dei
import derived_soak as dsoak
import gmc_blobs_inputs as gbi
from scan_checks import assert_counts_equal, device_centres_of, to_device
from test_gpu_blobs import assert_outputs, device_blobs
from test_gpu_derived_edges import shifted
from test_gpu_gmc import assert_info_equal
from test_gpu_gmc_blobs import assert_blobs, assert_info, device_scan, keep_tensor, soff_tensor

pytestmark = pytest.mark.gpu

JUNK, JUNK_FLAG = -7, 9
LAYOUT_NAMES = {False: "40-byte", True: "compact"}


def device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact):
    """Through mtgpu_scan_gmc_device into junk-filled outputs -> (flags, centres uint32, info GMC_INFO_DTYPE) on the host."""
    import torch
    F = d_off.numel() - 1
    fl = torch.full((F,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce = torch.full((F,), JUNK, dtype=torch.int32, device="cuda")
    inf = torch.full((F, 5), JUNK, dtype=torch.int32, device="cuda")
    s.scan_gmc_device(d_rec, d_off, d_sd, ms, q8, compact=compact, flags=fl, centres=ce, info=inf)
    torch.cuda.synchronize()
    return fl.cpu().numpy(), ce.cpu().numpy().view(np.uint32), inf.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)


def assert_gmc(s, p, d_rec, d_off, d_sd, compact, mv, off, sd, ms, what):
    """mtgpu_scan_gmc_device against derived_soak.gmc_counts_np: flags, centres and every info field."""
    want_c, want_i = dsoak.gmc_counts_np(p, mv, off, sd, ms, bei.Q8)
    fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, ms, bei.Q8, compact)
    assert_counts_equal(ce, want_c, what, got_f=fl, want_f=(want_c >= max(1, p.clusters_needed)).astype(np.uint8))
    assert_info_equal(info, want_i, what)


def pick(r, frames):
    return {k: np.asarray(v)[list(frames)] for k, v in r.items()}


# ------------------------------------------------------------------ a. head, step boundary and tail, resident forms

@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_blob_scan_head_step_boundary_and_tail(gpu_scanner_factory, vn):
    """blobs_frames_kernel<COMPACT, MASKED, PIPE = false>, all four: dei.edge_batch() (first records on all 16 residues of
    a 128-byte line; frames as long as the head peel - 1 / 0 / + 1 and the head plus one or two steps - 1 / 0 / + 1 / + 2)
    without a mask and in two streams under all-ones keeps.  Cell A holds exactly three voters on the positions a wrong
    loop bound drops or reads twice: 2 centres, one blob of 2 and the box of A + N at level 3 (a dropped voter: nothing),
    nothing at level 4 (a voter read twice: the pair)."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    p = bei.edge_params(vn)
    s = gpu_scanner_factory(p)
    hand, want = bei.edge_hand(vn), bei.edge_model(vn)
    d_soff, d_keep = soff_tensor(bei.edge_soff()), keep_tensor(bei.ones_keeps(p, 2))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        assert d_rec.data_ptr() % 128 == 0                           # what head_of() assumes of a fresh allocation
        centres = device_centres_of(s, d_rec, d_off, d_sd, compact)[1]
        for masked in (False, True):
            what = f"vn {vn}, {LAYOUT_NAMES[compact]}, {'all-ones keeps' if masked else 'no mask'}"
            got = device_blobs(s, d_rec, d_off, d_sd, compact, 2, *((d_soff, d_keep) if masked else (None, None)))
            assert_outputs(got, hand, what + ", by hand", p, 2)
            assert_outputs(got, want, what + ", the model", p, 2)
            assert_counts_equal(got["centres"], centres, what + ", mtgpu_scan_centres_device")


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_compensated_blob_scan_head_step_boundary_and_tail(gpu_scanner_factory, vn):
    """gmc_blobs_frames_kernel<COMPACT, MASKED> at max_shift 0 on the same batch, without d_keep (the unmasked estimate)
    and under all-ones keeps (the masked estimate, which stages a keep word per record) — each followed by the residual
    vote's own pass over the records.  The five blob outputs by hand and by the model; info on every frame: n_in, n_x and
    n_y are exact record counts of the estimate pass."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    p = bei.edge_params(vn)
    s = gpu_scanner_factory(p)
    hand = bei.edge_hand(vn)
    d_soff, d_keep = soff_tensor(bei.edge_soff()), keep_tensor(bei.ones_keeps(p, 2))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        centres = device_centres_of(s, d_rec, d_off, d_sd, compact)[1]
        for masked in (False, True):
            what = f"max_shift 0, vn {vn}, {LAYOUT_NAMES[compact]}, {'all-ones keeps' if masked else 'no keep'}"
            want = bei.edge_gmc_model(vn, False, 0, masked)
            got = device_scan(s, d_rec, d_off, d_sd, compact, 0, bei.Q8, 2, *((d_soff, d_keep) if masked else (None, None)))
            assert_blobs(got, hand, what + ", by hand", p, 2)
            assert_blobs(got, want, what + ", the model", p, 2)
            assert_info(got, want["info"], what)
            assert_counts_equal(got["centres"], centres, what + ", mtgpu_scan_centres_device")


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_compensated_blob_scan_of_the_pan_moved_edge_batch(gpu_scanner_factory, vn):
    """The edge batch with every src moved by (-7, +3): lengths and residues stay, every still record now carries the pan
    (7, -3).  max_shift 16, min_share_q8 128, without a keep and under all-ones keeps: all six outputs against the model;
    on the 44 long test frames the pan is found and the hand values hold — a record lost or doubled by the estimate
    shows in n_in, n_x, n_y, one lost or doubled by the residual vote in the pair."""
    mv, off, sd = bei.pan_batch()
    p = bei.edge_params(vn)
    s = gpu_scanner_factory(p)
    long = bei.long_test_frames()
    hand = bei.edge_hand(vn, long)
    d_soff, d_keep = soff_tensor(bei.edge_soff()), keep_tensor(bei.ones_keeps(p, 2))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for masked in (False, True):
            what = f"pan {bei.PAN}, vn {vn}, {LAYOUT_NAMES[compact]}, {'all-ones keeps' if masked else 'no keep'}"
            want = bei.edge_gmc_model(vn, True, bei.MS, masked)
            got = device_scan(s, d_rec, d_off, d_sd, compact, bei.MS, bei.Q8, 2, *((d_soff, d_keep) if masked else (None, None)))
            assert_blobs(got, want, what + ", the model", p, 2)
            assert_info(got, want["info"], what)
            assert_blobs(pick(got, long), hand, what + ", the long frames by hand")
            assert (got["info"][long][:, :2] == bei.PAN).all(), what


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_compensated_scan_head_step_boundary_and_tail(gpu_scanner_factory, vn):
    """gmc_frames_kernel's resident form on the edge batch (max_shift 0 and 16) and on the pan-moved one (16): flags,
    centres and info against derived_soak.gmc_counts_np; the hand counts on the frames where they hold."""
    p = bei.edge_params(vn)
    s = gpu_scanner_factory(p)
    emv, off, sd, test, _, _ = dei.edge_batch()
    pmv = bei.pan_batch()[0]
    long = bei.long_test_frames()
    for compact in (False, True):
        for name, mv, settings in (("edge batch", emv, (0, bei.MS)), ("pan-moved", pmv, (bei.MS,))):
            d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
            for ms in settings:
                what = f"{name}, max_shift {ms}, vn {vn}, {LAYOUT_NAMES[compact]}"
                assert_gmc(s, p, d_rec, d_off, d_sd, compact, mv, off, sd, ms, what)
                ce = device_gmc(s, d_rec, d_off, d_sd, ms, bei.Q8, compact)[1]
                frames = long if mv is pmv else list(test) if ms == 0 else []
                assert ce[frames].tolist() == bei.edge_hand(vn, frames)["centres"].tolist(), what


# ------------------------------------------------------------------ b. the same batch through the pipe forms

PIPE_LAYOUTS = [m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY, m.LAYOUT_AOS40]
PIPE_FRAMES, PIPE_RECORDS = 137, 450000


def run_one_submit(pipe, frames):
    """Feed every frame, assert that they wait in ONE batch, drain -> (flags, counts) in tag order."""
    for i, f in enumerate(frames):
        pipe.feed(f, float(i), tag=i)
    assert pipe._inflight == 0 and pipe._lib.mtgpu_batch_frames(pipe._cur) == len(frames)
    out = pipe.drain_centres()
    assert [t for _, _, t, _ in out] == list(range(len(frames)))
    return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]


@pytest.mark.parametrize("layout", PIPE_LAYOUTS, ids=["compact8-zero-copy", "aos40"])
def test_edge_batch_through_the_pipe_forms(gpu_scanner_factory, layout):
    """One pipe with room for the whole edge batch in one submit (137 frames, 443 572 records), so every frame keeps its
    residue: the staging block starts on a page and its record area behind a header of (9 x 138 + 63) & ~63 = 1280
    bytes, ten 128-byte lines.  blobs_frames_kernel<…, PIPE = true> without a mask and under an all-ones keep
    (set_blobs(2, "largest") and set_blobs(1, "centres")); gmc_frames_kernel's pipe form with set_gmc(16, 128, "vector")
    on the pan-moved batch and set_gmc(0, …) on the original, both without a mask and under the all-ones keep.  Flags
    and counts against the resident models."""
    emv, off, sd, test, _, _ = dei.edge_batch()
    assert len(off) - 1 == PIPE_FRAMES and len(emv) <= PIPE_RECORDS and ((9 * (PIPE_FRAMES + 1) + 63) & ~63) % 128 == 0
    frames, moved = bei.pipe_frames(False), bei.pipe_frames(True)
    long = bei.long_test_frames()
    for vn in bei.EDGE_VN:
        p = bei.edge_params(vn)
        cn = max(1, p.clusters_needed)
        s = gpu_scanner_factory(p)
        want = bei.edge_model(vn)
        hand = bei.edge_hand(vn)
        assert want["centres"].tolist() == hand["centres"].tolist() and want["largest"].tolist() == hand["largest"].tolist()
        with contextlib.closing(m.ScanPipe(s, PIPE_RECORDS, PIPE_FRAMES, 1, layout=layout, centres=True)) as pipe:
            for keep in (None, bei.ones_keeps(p)[0]):
                what = f"vn {vn}, keep {'all ones' if keep is not None else 'none'}"
                pipe.set_keep(keep)
                assert pipe.has_keep == (keep is not None)
                # the blob scan's pipe form
                pipe.set_blobs(2, "largest")
                fl, co = run_one_submit(pipe, frames)
                assert co == hand["largest"].tolist(), what
                assert fl == bm.flags_np(p, hand["centres"], hand["largest"], 2).tolist(), what
                pipe.set_blobs(1, "centres")
                fl, co = run_one_submit(pipe, frames)
                assert co == hand["centres"].tolist(), what
                assert fl == bm.flags_np(p, hand["centres"], hand["largest"], 1).tolist(), what
                pipe.set_blobs(0)
                # the compensated scan's pipe form: the pan-moved batch, then the original at max_shift 0
                gm_want = bei.edge_gmc_model(vn, True, bei.MS, keep is not None)
                vectors = [(int(r[0]) & 0xFFFF) | ((int(r[1]) & 0xFFFF) << 16) for r in gm_want["info"]]
                pipe.set_gmc(bei.MS, bei.Q8, "vector")
                fl, co = run_one_submit(pipe, moved)
                assert co == vectors, what
                assert fl == (gm_want["centres"] >= cn).astype(int).tolist(), what
                assert [m.ScanPipe.unpack_gmc_vector(co[f]) for f in long] == [bei.PAN] * len(long), what
                pipe.set_gmc(bei.MS, bei.Q8, "centres")
                fl, co = run_one_submit(pipe, moved)
                assert co == gm_want["centres"].tolist(), what
                assert [co[f] for f in long] == bei.edge_hand(vn, long)["centres"].tolist(), what
                pipe.set_gmc(0, bei.Q8, "centres")
                fl, co = run_one_submit(pipe, frames)
                assert co == hand["centres"].tolist() and fl == (hand["centres"] >= cn).astype(int).tolist(), what
                pipe.set_gmc(0, bei.Q8, "vector")
                fl, co = run_one_submit(pipe, frames)
                assert co == [0] * PIPE_FRAMES and fl == (hand["centres"] >= cn).astype(int).tolist(), what
                pipe.clear_gmc()


# ------------------------------------------------------------------ c. 40-byte records on a base shifted by 4, 12 and 20 bytes

def test_unaligned_40_byte_base(gpu_scanner_factory):
    """(base & 7) != 0 takes stream_mv40's branch without a head peel, in every pass of every kernel: the blob scan
    without a mask and under all-ones keeps, the compensated blob scan at max_shift 0 and 16 without a keep and under a
    random 85 % keep (its masked estimate looks the keep bit up per record), and the compensated scan — at byte shifts 4,
    12 and 20, against the models."""
    import torch
    mv, off, sd = dei.unaligned_batch()
    p = bei.unaligned_params()
    s = gpu_scanner_factory(p)
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    _, d_off, d_sd = to_device(mv[:0], off, sd, False)
    d_soff = soff_tensor(bei.UNALIGNED_SOFF)
    keeps = {k: keep_tensor(bei.unaligned_keeps(k)) for k in ("ones", "random")}
    for shift in dei.UNALIGNED_SHIFTS:
        d_rec = shifted(raw, shift)
        for keep in (None, "ones"):
            got = device_blobs(s, d_rec, d_off, d_sd, False, 2, *((d_soff, keeps[keep]) if keep else (None, None)))
            assert_outputs(got, bei.unaligned_model(None, keep), f"blob scan, base shifted by {shift} bytes, keep {keep}", p, 2)
        for ms in bei.UNALIGNED_SHIFT_SETTINGS:
            for keep in (None, "random"):
                what = f"compensated blob scan, max_shift {ms}, base shifted by {shift} bytes, keep {keep}"
                want = bei.unaligned_model(ms, keep)
                got = device_scan(s, d_rec, d_off, d_sd, False, ms, bei.Q8, 2, *((d_soff, keeps[keep]) if keep else (None, None)))
                assert_blobs(got, want, what, p, 2)
                assert_info(got, want["info"], what)
            assert_gmc(s, p, d_rec, d_off, d_sd, False, mv, off, sd, ms, f"compensated scan, max_shift {ms}, base shifted by {shift} bytes")


# ------------------------------------------------------------------ d. squares at and beyond 2^32

@pytest.mark.parametrize("thr", dei.BIG_ACTIVITY_THRESHOLDS)
def test_magnitude_beyond_32_bits(gpu_scanner_factory, thr):
    """dei.big_frames(): |d|^2 at and above 2^32, thresholds on both sides, through the blob scan's vote and — at
    max_shift 0 — through the compensated blob scan's residual square, which is code of its own.  Centres from exact
    Python integers; blobs, largest and box from the model (one blob of one cell wherever the count is 1)."""
    mv, off, sd = dei.big_frames()
    seen = set()
    for vn in bei.BIG_VN:
        p = bei.big_params(thr, vn)
        hand = bei.big_hand(thr, vn)
        want = bm.model_batch(p, mv, off, sd)
        seen |= set(hand["centres"])
        s = gpu_scanner_factory(p)
        for compact in (False, True):
            what = f"threshold {thr} vn {vn}, {LAYOUT_NAMES[compact]}"
            d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
            got = device_blobs(s, d_rec, d_off, d_sd, compact, 1)
            assert got["centres"].tolist() == hand["centres"], what
            assert_outputs(got, want, "blob scan, " + what, p, 1)
            got = device_scan(s, d_rec, d_off, d_sd, compact, 0, bei.Q8, 1)
            assert got["centres"].tolist() == hand["centres"], what
            assert_blobs(got, want, "compensated blob scan, " + what, p, 1)
            assert not got["info"][:, :4].any()
    assert thr > 8.5e9 or seen == {0, 1}


def test_residual_square_beyond_32_bits_under_a_pan(gpu_scanner_factory):
    """bei.pan_big_frames(): a record that moves by 65 535 under a pan of -127 on the same axis, once per axis.  The
    residual 65 662 squares to 4 311 498 244 >= 2^32 (16 530 948 if cut to 32 bits) where 65 535^2 stays below: at the
    threshold 2^32 the frame has its centres iff the pan is applied and the square is kept whole.  All values from exact
    Python integers (bei.pan_big_hand); max_shift 0 on the same frames reads nothing."""
    mv, off, sd = bei.pan_big_frames()
    p = bei.big_params(bei.PAN_BIG_THR, bei.PAN_BIG_VN)
    s = gpu_scanner_factory(p)
    ones = keep_tensor(bei.ones_keeps(p))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for ms in (bei.PAN_BIG_MS, 0):
            hand, info = bei.pan_big_hand(ms)
            for masked in (False, True):
                what = f"max_shift {ms}, {LAYOUT_NAMES[compact]}, masked {masked}"
                got = device_scan(s, d_rec, d_off, d_sd, compact, ms, bei.Q8, 1, *((soff_tensor([0, 2]), ones) if masked else (None, None)))
                assert_blobs(got, hand, what, p, 1)
                assert_info(got, info, what)
            fl, ce, inf = device_gmc(s, d_rec, d_off, d_sd, ms, bei.Q8, compact)
            assert ce.tolist() == hand["centres"], what
            assert_info_equal(inf, np.array(info, dtype=np.int64), what)
