"""GPU tier (`-m gpu`): ignore zones — the masked centre scan (include/mtgpu_zones.h, csrc/zones_kernels.hip).

Expected values: mtgpu_scan_centres_device (existing code) for the all-ones mask; the unchanged oracle on filtered
records for vectors_needed >= 1; numbers written out by hand in tests/zones_inputs.py for the word seams,
vectors_needed == 0 and the stream lookup.  tests/test_zones_host.py holds all of them against each other without a
GPU.  Every comparison is exact; outputs are pre-filled with junk: every element must be written by the call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, tune, zones

import derived_edge_inputs as dei
import oracle_binding as ob
import zones_inputs as zi
from golden_cases import load_hand_cases
from scan_checks import assert_counts_equal, device_centres_of, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG = -7, 9


# ------------------------------------------------------------------ device helpers

def soff_tensor(stream_off):
    import torch
    return torch.from_numpy(np.asarray(stream_off).astype(np.int64)).cuda()


def keep_tensor(keeps):
    """bool [S, gh, gw] -> int64 [S, gh, W] on the device (the bits of the uint64 words)."""
    import torch
    return torch.from_numpy(zi.pack_keeps(keeps).view(np.int64).copy()).cuda()


def device_zones(s, d_rec, d_off, d_sd, d_soff, d_keep, compact, want_all=True, stream=None):
    """Through mtgpu_scan_zones_device into junk-filled outputs -> (flags uint8, centres uint32, centres_all uint32 or
    None) on the host."""
    import torch
    n = d_off.numel() - 1
    fl = torch.full((n,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    ca = torch.full((n,), JUNK, dtype=torch.int32, device="cuda") if want_all else None
    torch.cuda.synchronize()
    s.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, compact=compact, flags=fl, centres=ce, centres_all=ca, stream=stream)
    torch.cuda.synchronize()
    return fl.cpu().numpy(), ce.cpu().numpy().view(np.uint32), None if ca is None else ca.cpu().numpy().view(np.uint32)


def zones_both_layouts(s, mv, off, sd, soff, keeps, what):
    """Both record layouts through the device entry point; yields (label, flags, centres, centres_all)."""
    d_soff, d_keep = soff_tensor(soff), keep_tensor(keeps)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        yield (f"{what}, {'compact' if compact else '40-byte'}",) + device_zones(s, d_rec, d_off, d_sd, d_soff, d_keep, compact)


def assert_is_the_centre_scan(s, mv, off, sd, what, hand=None, n_streams=1):
    """With an all-ones mask centres, centres_all and flags are mtgpu_scan_centres_device's, on both layouts; `hand`:
    the counts derived by hand.  The frames are dealt to n_streams streams (the result cannot depend on it)."""
    F = len(off) - 1
    soff = np.round(np.linspace(0, F, n_streams + 1)).astype(np.uint64)
    keeps = np.ones((n_streams, s.params.grid_h, s.params.grid_w), dtype=bool)
    d_soff, d_keep = soff_tensor(soff), keep_tensor(keeps)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        want_f, want_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        fl, ce, ca = device_zones(s, d_rec, d_off, d_sd, d_soff, d_keep, compact)
        label = f"{what}, {'compact' if compact else '40-byte'}"
        assert_counts_equal(ce, want_c, label + " centres", got_f=fl, want_f=want_f)
        assert_counts_equal(ca, want_c, label + " centres_all")
        if hand is not None:
            assert_counts_equal(ce, hand, label + " against the hand values")
    return want_c


# ------------------------------------------------------------------ 1. the all-ones mask is the centre scan

def test_hand_cases_with_a_full_mask(gpu_scanner_factory):
    """The 30 hand-derived check_frame cases, each alone, under its own VECTORS_NEEDED, 0 and 255."""
    _, cases = load_hand_cases()
    assert len(cases) == 30
    scanners = {}
    nonzero = 0
    for name, kw, case in cases:
        mv, off, sd, hand = dei.hand_case_batch(case)
        for vn in (kw["vectors_needed"], 0, 255):
            key = tuple(sorted(dict(kw, vectors_needed=vn).items()))
            if key not in scanners:
                scanners[key] = gpu_scanner_factory(m.ScanParams.from_config(**dict(key)))
            got = assert_is_the_centre_scan(scanners[key], mv, off, sd, f"{name} vn {vn}", [hand] if vn == kw["vectors_needed"] else None)
            nonzero += int(got[0] > 0)
    assert nonzero == 45                                             # (CPU: the oracle's counts of the same 90 scans)


def test_hand_cases_as_one_batch_with_a_full_mask(gpu_scanner_factory):
    base, mv, off, sd, hand = dei.hand_base_batch()
    assert sum(1 for h in hand if h) >= 5
    s = gpu_scanner_factory(m.ScanParams.from_config(**base))
    assert_is_the_centre_scan(s, mv, off, sd, "hand cases, one batch", hand, n_streams=3)


@pytest.mark.parametrize("vn", [3, 4])
def test_head_step_boundary_and_tail_with_a_full_mask(gpu_scanner_factory, vn):
    """dei.edge_batch(): first records on all 16 residues of a 128-byte line, frames as long as the head peel -1/0/+1 and
    the head plus one or two steps -1/0/+1/+2.  Cell A holds exactly three voters on the positions a wrong loop bound
    drops or reads twice: 2 centres at level 3, 0 at level 4."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    hand = dei.edge_hand_sweep()[1, vn - 3]                          # threshold 4
    assert int(hand.sum()) == (2 * len(test) if vn == 3 else 0)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, mv_threshold_sq=4.0, vectors_needed=vn))
    d_rec, _, _ = to_device(mv[:16], off[:2], sd[:1], False)
    assert d_rec.data_ptr() % 128 == 0                               # what head_of() assumes of a fresh allocation
    assert_is_the_centre_scan(s, mv, off, sd, f"head / step / tail vn {vn}", hand, n_streams=2)


def test_unaligned_40_byte_base_with_a_full_mask(gpu_scanner_factory):
    """(base & 7) != 0 takes stream_mv40's branch without a head peel: byte shifts 4, 12, 20 against the oracle."""
    import torch
    from test_gpu_derived_edges import shifted
    mv, off, sd = dei.unaligned_batch()
    p = m.ScanParams.from_config(1920, 1080)
    want_f, want_c = ob.scan_centres(p, mv, off, sd, nthreads=4)
    assert int((want_c > 0).sum()) > 20
    s = gpu_scanner_factory(p)
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    _, d_off, d_sd = to_device(mv[:0], off, sd, False)
    d_soff, d_keep = soff_tensor([0, 13, 40]), keep_tensor(np.ones((2, 68, 120), dtype=bool))
    for shift in dei.UNALIGNED_SHIFTS:
        fl, ce, ca = device_zones(s, shifted(raw, shift), d_off, d_sd, d_soff, d_keep, False)
        assert_counts_equal(ce, want_c, f"base shifted by {shift} bytes", got_f=fl, want_f=want_f)
        assert_counts_equal(ca, want_c, f"base shifted by {shift} bytes, centres_all")


@pytest.mark.parametrize("thr", dei.BIG_ACTIVITY_THRESHOLDS)
def test_magnitude_beyond_32_bits_with_a_full_mask(gpu_scanner_factory, thr):
    """dei.big_frames(): |d|^2 at and above 2^32, thresholds on both sides; counts from exact Python integers."""
    mv, off, sd = dei.big_frames()
    seen = set()
    for vn in (1, 2):
        hand = dei.big_hand_count(thr, vn)
        seen |= set(hand)
        s = gpu_scanner_factory(m.ScanParams.from_config(32768, 32768, mv_threshold_sq=thr, vectors_needed=vn, **dei.BIG_KW))
        assert_is_the_centre_scan(s, mv, off, sd, f"threshold {thr} vn {vn}", hand)
    assert thr > 8.5e9 or seen == {0, 1}


# ------------------------------------------------------------------ 2. random masks against the oracle on filtered records

@pytest.mark.parametrize("i", range(len(zi.RANDOM_CASES)), ids=["%dx%d-mask%g-vn%d" % c for c in zi.RANDOM_CASES])
def test_random_masks_against_the_oracle_on_filtered_records(gpu_scanner_factory, i):
    p, mv, off, sd, soff, keeps = zi.random_case(i)
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert zi.counts_to_count(want_c, want_all, off, sd)
    s = gpu_scanner_factory(p)
    for label, fl, ce, ca in zones_both_layouts(s, mv, off, sd, soff, keeps, "random masks"):
        assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
        assert_counts_equal(ca, want_all, label + " centres_all")
    # has_sd == NULL: side data iff records (here: every frame), through the host entry point
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, None, soff, keeps)
    fl, ce, ca = s.scan_zones(m.FrameBatch(mv, off, None, None), soff, zi.pack_keeps(keeps), want_all=True)
    assert_counts_equal(ce, want_c, "has_sd NULL, host entry", got_f=fl, want_f=want_f)
    assert_counts_equal(ca, want_all, "has_sd NULL, host entry, centres_all")


# ------------------------------------------------------------------ 3. word seams

def test_word_seams_by_hand(gpu_scanner_factory):
    """gw = 130, W = 3: runs across both word boundaries and a vertical pair; one cell cleared per stream.  The carry
    into a neighbouring word must come from the masked word."""
    p, mv, off, sd, soff, keeps, hand, hand_all = zi.seam_case()
    s = gpu_scanner_factory(p)
    for label, fl, ce, ca in zones_both_layouts(s, mv, off, sd, soff, keeps, "word seams"):
        assert_counts_equal(ce, hand, label, got_f=fl, want_f=(hand >= 1).astype(np.uint8))
        assert_counts_equal(ca, hand_all, label + " centres_all")


# ------------------------------------------------------------------ 4. vectors_needed == 0

@pytest.mark.parametrize("margin", [0, 1])
def test_vectors_needed_zero_by_hand(gpu_scanner_factory, margin):
    """Frames with side data and no record: every kept analysed cell is active, an ignored one is not; a margin row is an
    active neighbour.  has_sd == NULL for the same frames: no record, no side data, 0 everywhere."""
    import torch
    p, off, sd, soff, keeps, hand, hand_all = zi.vn0_case(margin)
    s = gpu_scanner_factory(p)
    none = np.zeros(0, dtype=m.MV_DTYPE)
    for label, fl, ce, ca in zones_both_layouts(s, none, off, sd, soff, keeps, f"vn 0 margin {margin}"):
        assert_counts_equal(ce, hand, label, got_f=fl, want_f=(hand >= 1).astype(np.uint8))
        assert_counts_equal(ca, hand_all, label + " centres_all")
    d_rec, d_off, _ = to_device(none, off, None, True)
    fl, ce, ca = device_zones(s, d_rec, d_off, None, soff_tensor(soff), keep_tensor(keeps), True)
    assert not fl.any() and not ce.any() and not ca.any()
    torch.cuda.synchronize()
    fl, ce, ca = s.scan_zones(m.FrameBatch(none, off, None, sd), soff, zi.pack_keeps(keeps), want_all=True)
    assert ce.tolist() == hand.tolist() and ca.tolist() == hand_all.tolist()


# ------------------------------------------------------------------ 5. the margin as a mask

def test_margin_as_a_mask(gpu_scanner_factory):
    """vn >= 1: VERTICAL_MASK 0 plus a mask that clears the strips equals VERTICAL_MASK 0.05 / 0.10 without a mask
    (mtgpu_scan_centres_device through those contexts), on 1080p frames whose motion reaches the strips."""
    mv, off, sd = zi.margin_case()
    s0 = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, vertical_mask=0.0))
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    all0 = device_centres_of(s0, d_rec, d_off, d_sd, True)[1]
    for vmask, margin in zi.MARGIN_MASKS:
        pm = m.ScanParams.from_config(1920, 1080, vertical_mask=vmask)
        assert pm.vertical_margin == margin
        want_f, want_c = device_centres_of(gpu_scanner_factory(pm), d_rec, d_off, d_sd, True)
        assert int((want_c < all0).sum()) >= 12 and int((want_c > 0).sum()) == 24
        strip = np.ones((1, 68, 120), dtype=bool)
        strip[0, :margin] = strip[0, 68 - margin:] = False
        fl, ce, ca = device_zones(s0, d_rec, d_off, d_sd, soff_tensor([0, 24]), keep_tensor(strip), True)
        assert_counts_equal(ce, want_c, f"margin {margin} as a mask", got_f=fl, want_f=want_f)
        assert_counts_equal(ca, all0, f"margin {margin} as a mask, centres_all")


# ------------------------------------------------------------------ 6. the stream lookup

def test_stream_lookup_by_hand(gpu_scanner_factory):
    """Six streams of 0, 1, 2, 0, 3 and 1 frames, every frame the same records, stream s keeps band s alone: the count
    names the stream.  Two frames behind stream_off[n_streams] read 0 on the device entry point."""
    p, mv, off, sd, soff, keeps, hand, hand_all = zi.lookup_case()
    s = gpu_scanner_factory(p)
    for label, fl, ce, ca in zones_both_layouts(s, mv, off, sd, soff, keeps, "stream lookup"):
        assert_counts_equal(ce, hand, label, got_f=fl, want_f=(hand >= 4).astype(np.uint8))
        assert_counts_equal(ca, hand_all, label + " centres_all")
    F = 7
    fl, ce, ca = s.scan_zones(m.FrameBatch(mv[:int(off[F])], off[:F + 1], None, sd[:F]), soff, zi.pack_keeps(keeps), want_all=True)
    assert ce.tolist() == hand[:F].tolist() and ca.tolist() == hand_all[:F].tolist()
    # the host entry point rejects offsets that do not end on n_frames
    with pytest.raises(m.MtgpuError) as ei:
        s.scan_zones(m.FrameBatch(mv, off, None, sd), soff, zi.pack_keeps(keeps))
    assert ei.value.code == _abi.MT_ERR_INVALID and "n_frames" in str(ei.value)


# ------------------------------------------------------------------ 7. exact writes

def test_exact_writes(gpu_scanner_factory):
    """Canaries on both sides of every output, every combination of NULL outputs, n_frames == 0, failing calls, and a
    non-default stream."""
    import torch
    p, mv, off, sd, soff, keeps = zi.random_case(0)
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    want = {"flags": want_f, "centres": want_c, "centres_all": want_all}
    s = gpu_scanner_factory(p)
    lib = s._lib
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_soff, d_keep = soff_tensor(soff), keep_tensor(keeps)
    F, PAD = len(off) - 1, 64
    NAMES = ("flags", "centres", "centres_all")

    def buffers():
        b = {"flags": torch.full((F + 2 * PAD,), JUNK_FLAG, dtype=torch.uint8, device="cuda")}
        for n in NAMES[1:]:
            b[n] = torch.full((F + 2 * PAD,), JUNK, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        return b

    def run(names, n_frames=F, rb=8, stream=None, ctx=None, over=None):
        b = buffers()
        ptr = {n: (b[n][PAD:].data_ptr() if n in names else None) for n in NAMES}
        ptr.update(over or {})
        rc = lib.mtgpu_scan_zones_device((ctx or s)._ctx, d_rec.data_ptr(), rb, len(mv), d_off.data_ptr(), d_sd.data_ptr(), n_frames,
                                         d_soff.data_ptr(), len(soff) - 1, d_keep.data_ptr(), ptr["flags"], ptr["centres"],
                                         ptr["centres_all"], stream)
        torch.cuda.synchronize()
        return rc, {n: t.cpu().numpy() for n, t in b.items()}

    def untouched(raw, names=NAMES):
        return all((raw[n] == (JUNK_FLAG if n == "flags" else JUNK)).all() for n in names)

    combos = [NAMES, ("flags", "centres"), ("flags", "centres_all"), ("centres", "centres_all"), ("flags",), ("centres",), ("centres_all",)]
    for names in combos:
        rc, raw = run(names)
        assert rc == _abi.MT_OK, (names, lib.mtgpu_last_error())
        for n in NAMES:
            junk = JUNK_FLAG if n == "flags" else JUNK
            assert (raw[n][:PAD] == junk).all() and (raw[n][PAD + F:] == junk).all(), (names, n)
            if n in names:
                got = raw[n][PAD:PAD + F]
                assert np.array_equal(got if n == "flags" else got.view(np.uint32), want[n]), (names, n)
            else:
                assert untouched(raw, (n,)), (names, n)
    # all three NULL
    rc, raw = run(())
    assert rc == _abi.MT_ERR_INVALID and "all NULL" in lib.mtgpu_last_error().decode() and untouched(raw)
    # n_frames == 0: MT_OK, nothing written
    rc, raw = run(NAMES, n_frames=0)
    assert rc == _abi.MT_OK and untouched(raw)
    fl, ce, ca = s.scan_zones(m.FrameBatch(mv[:0], off[:1], None, None), [0, 0], zi.pack_keeps(keeps[:1]), want_all=True)
    assert len(fl) == len(ce) == len(ca) == 0
    # failing calls touch no byte: rec_bytes, an output in pinned host memory, the keep mask in pinned host memory, an
    # unsupported grid
    for rb in (0, 16, 41):
        rc, raw = run(NAMES, rb=rb)
        assert rc == _abi.MT_ERR_INVALID and "rec_bytes" in lib.mtgpu_last_error().decode() and untouched(raw)
    pinned = torch.full((F,), JUNK, dtype=torch.int32).pin_memory()
    for name in ("centres", "centres_all", "flags"):
        rc, raw = run(NAMES, over={name: pinned.data_ptr()})
        assert rc == _abi.MT_ERR_INVALID and ("d_" + name + " is not memory of device") in lib.mtgpu_last_error().decode()
        assert untouched(raw) and int((pinned != JUNK).sum()) == 0
    pinned_keep = torch.from_numpy(zi.pack_keeps(keeps).view(np.int64).copy()).pin_memory()
    b = buffers()
    rc = lib.mtgpu_scan_zones_device(s._ctx, d_rec.data_ptr(), 8, len(mv), d_off.data_ptr(), d_sd.data_ptr(), F, d_soff.data_ptr(),
                                     len(soff) - 1, pinned_keep.data_ptr(), b["flags"].data_ptr(), b["centres"].data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "d_keep is not memory of device" in lib.mtgpu_last_error().decode()
    assert untouched({n: t.cpu().numpy() for n, t in b.items()})
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    rc, raw = run(NAMES, ctx=big)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in lib.mtgpu_last_error().decode() and untouched(raw)
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_zones(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)), [0, 1],
                       np.zeros((1, 540, 15), dtype=np.uint64))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # a non-default stream
    st = torch.cuda.Stream()
    rc, raw = run(NAMES, stream=st.cuda_stream)
    assert rc == _abi.MT_OK
    assert np.array_equal(raw["centres"][PAD:PAD + F].view(np.uint32), want_c) and np.array_equal(raw["flags"][PAD:PAD + F], want_f)
    assert np.array_equal(raw["centres_all"][PAD:PAD + F].view(np.uint32), want_all)


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    p, mv, off, sd, soff, keeps = zi.random_case(10)
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    s.profile(True)
    try:
        s.profile_read()
        fl, ce, ca = device_zones(s, d_rec, d_off, d_sd, soff_tensor(soff), keep_tensor(keeps), False)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert ce.tolist() == zi.oracle_batch(p, mv, off, sd, soff, keeps)[1].tolist()


# ------------------------------------------------------------------ 8. two-kernel planning

def test_two_kernel_planning(gpu_scanner_factory):
    """40 000 frames of 4 records: more planning blocks than the fused plan takes, so plan_count_kernel runs ahead of the
    scatter.  Two streams with random masks, every 7th frame without side data, against the oracle on filtered records."""
    p, mv, off, sd, soff, keeps = zi.plan_case()
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    s = gpu_scanner_factory(p)
    for label, fl, ce, ca in zones_both_layouts(s, mv, off, sd, soff, keeps, "40 000 frames"):
        assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
        assert_counts_equal(ca, want_all, label + " centres_all")


# ------------------------------------------------------------------ 9. downstream

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def downstream_input():
    """Three streams of 40 frames at 25 fps on the 1080p grid: an object (three cells: 3 centres) in six of every twenty
    frames, a pair of cells (2 centres) in every tenth frame and, in every frame, a clock (cells 110 .. 113 of row 4: 4
    centres) that the masks of streams 0 and 1 ignore — stream 2 keeps it.  Counts: 0, 2, 3 under the zones; 4, 6, 7 and
    (frame 9 of stream 2: object and pair) 9 with the clock."""
    S, F = 3, 40
    frames = []
    for st in range(S):
        for f in range(F):
            cells = [(110 + c, 4, 2, 5, 0) for c in range(4)]
            if (f + 7 * st) % 20 < 6:
                cells += [(40 + c + st, 30, 2 + c, 5, 0) for c in range(3)]
            if f % 10 == 9:
                cells += [(70, 50, 2, 5, 0), (71, 50, 2, 5, 0)]
            frames.append(dei.voters(cells))
    b = m.FrameBatch.from_frames(frames)
    pts = np.tile(np.arange(F, dtype=np.float64) / 25.0, S)
    keeps = np.ones((S, 68, 120), dtype=bool)
    keeps[:2, 4, 110:114] = False
    soff = np.arange(S + 1, dtype=np.uint64) * F
    return dei.frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
                      np.ones(S * F, dtype=np.uint8), pts, soff, keeps)


def test_downstream_merge_and_sweep(gpu_scanner_factory, downstream_input):
    """flags through mtgpu_merge_streams_device equal the oracle's merge of the filtered scan; centres through
    mtgpu_sweep_streams_device at levels 1, 2 and 4 equal the merge of flags_from_centres at each level."""
    import torch
    mv, off, sd, pts, soff, keeps = downstream_input
    S, F, CAP = 3, 40, 16
    p = m.ScanParams.from_config(1920, 1080, clusters_needed=2)
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert sorted(set(want_c.tolist())) == [0, 2, 3, 4, 6, 7, 9] and 0 < int(want_f[:F].sum()) < F and int(want_f[2 * F:].sum()) == F
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    d_pts, d_soff = torch.from_numpy(pts.copy()).cuda(), soff_tensor(soff)
    mps = [m.MergeParams(duration=F / 25.0, max_gap_sec=0.2, padding_sec=0.04, min_savings_pct=5.0) for _ in range(S)]
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    fl, ce, ca = s.scan_zones_device(d_rec, d_off, d_sd, d_soff, keep_tensor(keeps), centres_all=True)
    seg, res = s.merge_streams_device(fl, d_pts, d_soff, d_mp, seg_cap=CAP)
    torch.cuda.synchronize()
    assert np.array_equal(fl.cpu().numpy(), want_f) and np.array_equal(ce.cpu().numpy().view(np.uint32), want_c)
    recs = m.results_from_bytes(res.cpu().numpy())
    seg_h = seg.cpu().numpy()
    n_seg = []
    for i in range(S):
        a, b = i * F, (i + 1) * F
        wseg, wres = ob.pool_and_merge(pts[a:b][want_f[a:b] != 0], mps[i], False)
        wrec = np.zeros(1, dtype=m.MERGE_RESULT_DTYPE)
        for k, v in wres.items():
            wrec[k] = v
        assert recs[i:i + 1].tobytes() == wrec.tobytes(), (i, recs[i], wres)
        k = int(wres["n_segments"])
        assert np.array_equal(bits(seg_h[i, :k, 0]), bits(wseg["start"])) and np.array_equal(bits(seg_h[i, :k, 1]), bits(wseg["end"]))
        n_seg.append(k)
    assert n_seg[0] >= 2 and n_seg[2] == 1                            # the zones cut stream 0 up; stream 2 keeps its clock
    LEVELS = [1, 2, 4]
    sseg, sres = s.sweep_streams_device(ce, d_pts, d_soff, d_mp, LEVELS, seg_cap=CAP)
    torch.cuda.synchronize()
    kept = []
    for li, lv in enumerate(LEVELS):
        f2 = s.flags_from_centres(ce, lv)
        seg_a, res_a = s.merge_streams_device(f2, d_pts, d_soff, d_mp, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(f2.cpu().numpy(), (want_c >= lv).astype(np.uint8))
        assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg_a.cpu().numpy())) and np.array_equal(sres[li].cpu().numpy(), res_a.cpu().numpy())
        kept.append(int(f2.sum()))
    assert kept[0] > kept[2] > 0


def test_entry_points_agree(gpu_scanner_factory, downstream_input):
    """mtgpu_scan_frames_zones (host pointers), MotionScanner.scan_zones with one mask for every stream, and the device
    entry point return the same."""
    mv, off, sd, pts, soff, keeps = downstream_input
    p = m.ScanParams.from_config(1920, 1080, clusters_needed=2)
    s = gpu_scanner_factory(p)
    want_f, want_c, want_all = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    fl, ce, ca = device_zones(s, d_rec, d_off, d_sd, soff_tensor(soff), keep_tensor(keeps), True)
    hf, hc, ha = s.scan_zones(m.FrameBatch(mv, off, None, sd), soff, zi.pack_keeps(keeps), want_all=True)
    assert hc.dtype == np.uint32 and hf.dtype == np.uint8
    assert_counts_equal(hc, want_c, "host entry", got_f=hf, want_f=want_f)
    assert_counts_equal(ce, hc, "device entry against host entry", got_f=fl, want_f=hf)
    assert_counts_equal(ha, want_all, "host entry centres_all")
    assert_counts_equal(ca, ha, "device entry centres_all")
    assert s.scan_zones(m.FrameBatch(mv, off, None, sd), soff, zi.pack_keeps(keeps))[2] is None
    # a window of a larger batch: offsets that do not start at 0
    F = 40
    wf, wc, wa = s.scan_zones(m.FrameBatch(mv, off[F:2 * F + 1], None, sd[F:2 * F]), [0, F], zones.pack_keep(keeps[1]), want_all=True)
    assert wc.tolist() == want_c[F:2 * F].tolist() and wa.tolist() == want_all[F:2 * F].tolist() and wf.tolist() == want_f[F:2 * F].tolist()
    # one [gh, W] mask stands for every stream
    one = np.broadcast_to(keeps[0], keeps.shape)
    bf, bc, _ = s.scan_zones(m.FrameBatch(mv, off, None, sd), soff, zones.pack_keep(keeps[0]))
    assert bc.tolist() == zi.oracle_batch(p, mv, off, sd, soff, one)[1].tolist()
    with pytest.raises(ValueError):
        s.scan_zones(m.FrameBatch(mv, off, None, sd), soff, np.zeros((2, 68, 2), dtype=np.uint64))


def test_end_to_end_command(gpu_scanner_factory, downstream_input, tmp_path, capsys):
    """A .mtmv of stream 0 written with mvfile, then `python -m mvtrim_amd.zones --json` in a fresh child process with
    the clock as an --ignore rectangle, and once more with --ignore-busy; --mask-npy through zones.main in this process: the counts equal the direct calls."""
    mv, off, sd, pts, soff, keeps = downstream_input
    F = 40
    frames = [mv[int(off[f]):int(off[f + 1])] for f in range(F)]
    path = str(tmp_path / "stream.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    p = m.ScanParams.from_config(1920, 1080)
    s = gpu_scanner_factory(p)
    batch, fpts, hdr = tune.load(path)
    assert batch.n_frames == F and hdr["width"] == 1920
    mp = m.MergeParams(duration=F / 25.0, max_gap_sec=0.2, padding_sec=0.04, min_savings_pct=5.0)
    keep, direct = zones.measure(s, batch, fpts, keeps[0], mp)
    want_f, want_c, want_all = zi.oracle_batch(p, mv[:int(off[F])], off[:F + 1], sd[:F], [0, F], keeps[:1])
    assert direct["with_zones"]["centres"] == int(want_c.sum()) and direct["without_zones"]["centres"] == int(want_all.sum())
    assert direct["with_zones"]["motion_frames"] == int(want_f.sum()) < direct["without_zones"]["motion_frames"] == F
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "mvtrim_amd.zones", path, "--json", "--max-gap-sec", "0.2", "--padding-sec", "0.04",
            "--min-savings-pct", "5"]
    saved = str(tmp_path / "mask.npy")
    # the clock's cells 110 .. 113 of row 4 in pixels, one pixel inside the blocks' outer edges
    out = subprocess.run(base + ["--ignore", "1761,65,1823,79", "--save-mask", saved], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert doc["with_zones"] == direct["with_zones"] and doc["without_zones"] == direct["without_zones"]
    assert doc["ignored_cells"] == 4 and doc["ignored_share"] == 4 / (62 * 120) and (doc["grid_w"], doc["grid_h"], doc["frames"]) == (120, 68, F)
    assert doc["with_zones"]["segments"] > doc["without_zones"]["segments"] == 1
    assert np.array_equal(np.load(saved), keeps[0])
    # --ignore-busy 0.9: the clock's cells are centres in every frame, nothing else is in more than 36 of 40
    saved2 = str(tmp_path / "busy.npy")
    out = subprocess.run(base + ["--ignore-busy", "0.9", "--save-mask", saved2], capture_output=True, text=True, env=env, cwd=ROOT,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    doc2 = json.loads(out.stdout)
    assert doc2["with_zones"] == direct["with_zones"] and doc2["without_zones"] == direct["without_zones"] and doc2["ignored_cells"] == 4
    assert np.array_equal(np.load(saved2), keeps[0])
    # --mask-npy, in this process: the saved mask again
    capsys.readouterr()
    assert zones.main(base[3:] + ["--mask-npy", saved]) == 0
    assert json.loads(capsys.readouterr().out)["with_zones"] == direct["with_zones"]


def test_plain_c_zones_example(tmp_path):
    """examples/zones_example.c: a clock ignored from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "zones_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "zones_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame 15: 7 centres without the zone, 3 with" in out.stdout
    assert "motion frames: 60 of 60 without the zone, 10 with" in out.stdout
