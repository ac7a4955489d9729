"""GPU tier (`-m gpu`): the record-level and plan-level edge cases of the scan's suite, held against the shared
streamers of csrc/record_stream.h (head peel, steps, tail) as each kernel instantiates them with its own vote —
sweep_frames_kernel (csrc/sweep_kernels.hip), activity_frames_kernel (csrc/activity_kernels.hip) — and, for the unaligned
base, against motion_scores_kernel's own loop (csrc/scalar_kernels.hip).

The inputs and the values derived by hand from their construction come from tests/derived_edge_inputs.py;
tests/test_derived_edges_host.py holds them against the oracle without a GPU.  Here every comparison is exact (integers,
bit patterns of the scores), no expected value comes from the code under test, outputs are pre-filled with junk, and a
case goes through the host entry and through the device entry on both record layouts where the kernel has both."""
import ctypes as C

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_edge_inputs as dei
import test_gpu_motion_scalar as ms
from golden_cases import id_of, load_hand_cases
from scan_checks import assert_counts_equal, to_device
from test_gpu_activity import (JUNK, assert_maps_equal, assert_oracle_identities, device_maps, junk_maps, model_maps,
                               soff_tensor)
from test_gpu_sweep import assert_sweep_parity, device_sweep, junk_out, oracle_sweep

pytestmark = pytest.mark.gpu


def assert_maps_parity(s, mv, off, sd, soff, want, what, runs=(0, 1), host=True):
    """The host entry and the device entry on 40-byte and on compact records, at every run_frames of `runs`."""
    if host:
        assert_maps_equal(s.activity_map(m.FrameBatch(mv, off, None, sd), soff), want, what + " host entry")
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for run in runs:
            got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), compact, run_frames=run)
            assert_maps_equal(got, want, f"{what} device entry, compact {compact}, run_frames {run}")


def plan_of(p, n_thr, n_vec):
    pv = m.sweep_preview(p, n_thr, n_vec)
    return pv["passes"], pv["thresholds_per_pass"]


# ------------------------------------------------------------------ A. every pass shape of the sweep

@pytest.mark.parametrize("name", list(dei.PASS_SHAPES))
def test_sweep_every_pass_shape(gpu_scanner_factory, name):
    """Passes of 1, 2, 3, 4, 5, 6, 7 and 8 thresholds between the cases (NT = 1, 2, 4, 8, padded with ~0 and full), the
    fold over up to 8 tiles and skipped for one, the full 8 x 8 block in one pass and in two: the oracle's counts in
    the caller's order of thresholds and levels, which is never the sorted one."""
    p, mv, off, sd, thr, vec, plan, want = dei.pass_shape_case(name)
    assert plan_of(p, len(thr), len(vec)) == plan
    s = gpu_scanner_factory(p)
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, name)


# ------------------------------------------------------------------ B. chunk seams

@pytest.mark.parametrize("name", list(dei.SEAM_GRIDS))
def test_sweep_chunk_seams(gpu_scanner_factory, name):
    """Phase 2 in several chunks of rows (64 x 600 cells: 146 of 600 rows per chunk; 4K without a vertical mask: 123 of
    135): a vertical pair of cells on EVERY row boundary of the grid, each cell's only active neighbour being the one
    across the boundary, so wherever the plan puts a seam the halo rows decide two centres; k = 1 + y % 8 votes per cell,
    so each of the eight levels sees another set of pairs.  Plus horizontal pairs across the 64-bit word boundaries on
    the last row of the first chunk.  Counts by hand (tests/derived_edge_inputs.py, seam_case)."""
    p, mv, off, sd, thr, vec, hand = dei.seam_case(name)
    ch, R, single, pv = dei.sweep_chunk_rows(p, len(thr), len(vec))
    print(name, "plan", pv, "chunk_rows", ch, "of", R, "a single chunk would take", single)
    assert pv["lds_bytes"] < single and ch < R                       # the chunked path, or the test says nothing
    s = gpu_scanner_factory(p)
    assert_sweep_parity(s, mv, off, sd, thr, vec, hand, name)


# ------------------------------------------------------------------ C. |d|^2 at and above 2^32

def test_sweep_magnitude_beyond_32_bits(gpu_scanner_factory):
    """The magnitudes and thresholds of test_scan_magnitude_beyond_32_bits on a 32 x 32 grid of 1024-pixel cells.  Both
    records of a BIG_D pair fall into the last column (|dx| >= 65 519 leaves no other), which is never a centre; column
    30 holds two helpers of |d|^2 = 8 456 505 346 and is a centre at level v iff the helpers pass and >= v of the pair
    do — from exact Python integers.  A magnitude or a threshold cut to 32 bits changes 1s into 0s or 0s into 1s at the
    thresholds around 2^32; above 8 456 505 346 every count is 0, which a threshold cut to 32 bits turns into 1."""
    p = m.ScanParams.from_config(32768, 32768, **dei.BIG_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (32, 32, 0)
    mv, off, sd = dei.big_frames()
    s = gpu_scanner_factory(p)
    seen = set()
    for call in dei.BIG_CALLS:
        hand = np.array([[dei.big_hand_count(t, 1), dei.big_hand_count(t, 2)] for t in call], dtype=np.uint32)
        seen |= {int(x) for x in hand.reshape(-1)}
        assert_sweep_parity(s, mv, off, sd, call, [1, 2], hand, f"thresholds {call}")
    assert seen == {0, 1}


@pytest.mark.parametrize("thr", dei.BIG_ACTIVITY_THRESHOLDS)
def test_activity_magnitude_beyond_32_bits(gpu_scanner_factory, thr):
    """The same frames through the activity map, one context per threshold and VECTORS_NEEDED 1 / 2: cell (31, 31) is
    active iff enough of the pair's magnitudes pass; planes and frames against the model, the centre sum by hand."""
    mv, off, sd = dei.big_frames()
    for vn in (1, 2):
        p = m.ScanParams.from_config(32768, 32768, mv_threshold_sq=thr, vectors_needed=vn, **dei.BIG_KW)
        want = model_maps(p, mv, off, sd, [0, 5], 0)
        hand = dei.big_hand_count(thr, vn)
        assert int(want[1].sum()) == sum(hand) and want[2].tolist() == [5]
        s = gpu_scanner_factory(p)
        got = s.activity_map(m.FrameBatch(mv, off, None, sd), [0, 5])
        assert int(got[1].sum(dtype=np.uint64)) == sum(hand)
        assert_maps_parity(s, mv, off, sd, [0, 5], want[:3], f"threshold {thr} vectors_needed {vn}")


# ------------------------------------------------------------------ D. head, step boundary and tail

def test_sweep_head_step_boundary_and_tail(gpu_scanner_factory):
    """68 frames whose first records sit on all 16 residues of a 128-byte line (both record sizes), as long as the head
    peel - 1, the head, the head + 1, and the head + one or two steps of the unrolled loop (4096 records of 40 bytes,
    8192 compact ones) - 1, + 0, + 1, + 2.  Cell A holds EXACTLY three voters, on the first and last records, around
    the head and around the step boundaries: thresholds 1 and 4 read 2 at level 3 (a dropped voter: 0) and 0 at level 4
    (a voter read twice: 2), threshold 6 reads 0."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    hand = dei.edge_hand_sweep()
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    d_rec, _, _ = to_device(mv[:16], off[:2], sd[:1], False)
    assert d_rec.data_ptr() % 128 == 0                               # what head_of() assumes of a fresh allocation
    assert_sweep_parity(s, mv, off, sd, dei.EDGE_THR, dei.EDGE_VEC, hand, "head / step / tail")


@pytest.mark.parametrize("vn", [3, 4])
def test_activity_head_step_boundary_and_tail(gpu_scanner_factory, vn):
    """The same batch in two streams: with VECTORS_NEEDED 3 cell A is active and a centre in every test frame, with 4 in
    none (its neighbour N, 4 .. 10 voters, stays active and loses its only active neighbour).  Maps by hand."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    ha, hc, hf, soff = dei.edge_hand_maps(vn)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, mv_threshold_sq=4.0, vectors_needed=vn))
    assert_maps_parity(s, mv, off, sd, soff, (ha, hc, hf), f"vectors_needed {vn}", runs=(0, 1, 8))


# ------------------------------------------------------------------ E. 40-byte records on a base that is only 4-byte aligned

def shifted(raw, shift):
    """The bytes of `raw` (a host uint8 tensor) in device memory at `shift` bytes behind an allocation's start."""
    import torch
    buf = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device="cuda")
    view = buf[shift:shift + raw.numel()]
    view.copy_(raw)
    assert view.data_ptr() % 8 == shift % 8 == 4
    return view


def test_sweep_unaligned_40_byte_base(gpu_scanner_factory):
    """(base & 7) != 0 takes stream_mv40's branch without a head peel: the oracle's counts at byte shifts 4, 12, 20; an
    odd base is MT_ERR_INVALID and launches nothing."""
    import torch
    mv, off, sd = dei.unaligned_batch()
    thr, vec = [4, 16], [1, 2]
    want = oracle_sweep(1920, 1080, {}, mv, off, sd, thr, vec)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    _, d_off, d_sd = to_device(mv[:0], off, sd, False)
    for shift in dei.UNALIGNED_SHIFTS:
        got = device_sweep(s, shifted(raw, shift), d_off, d_sd, thr, vec, False)
        assert_counts_equal(got.reshape(-1), want.reshape(-1), f"base shifted by {shift} bytes")
    out = junk_out(2, 2, 40)
    odd = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")[1:1 + raw.numel()]
    rc = s._lib.mtgpu_scan_sweep_device(s._ctx, odd.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), 40,
                                        (C.c_double * 2)(*thr), 2, (C.c_int32 * 2)(*vec), 2, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in s._lib.mtgpu_last_error().decode() and int((out != JUNK).sum()) == 0


def test_activity_unaligned_40_byte_base(gpu_scanner_factory):
    import torch
    mv, off, sd = dei.unaligned_batch()
    soff = np.array([0, 13, 40], dtype=np.uint64)
    p = m.ScanParams.from_config(1920, 1080)
    want = model_maps(p, mv, off, sd, soff, 0)
    assert_oracle_identities(p, mv, off, sd, soff, 0, want[1], want[2], "model")
    assert int(want[1].sum()) > 0
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    aligned = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), False)
    assert_maps_equal(aligned, want[:3], "aligned base")
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    for shift in dei.UNALIGNED_SHIFTS:
        for run in (0, 1):
            got = device_maps(s, shifted(raw, shift), d_off, d_sd, soff_tensor(soff), False, run_frames=run)
            assert_maps_equal(got, aligned, f"base shifted by {shift} bytes against the aligned call, run_frames {run}")
            assert_maps_equal(got, want[:3], f"base shifted by {shift} bytes, run_frames {run}")
    outs = junk_maps(s, 2)
    odd = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")[1:1 + raw.numel()]
    d_soff = soff_tensor(soff)
    rc = s._lib.mtgpu_activity_map_device(s._ctx, odd.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), 40,
                                          d_soff.data_ptr(), 2, 0, 0, outs["active"].data_ptr(), outs["centre"].data_ptr(),
                                          outs["frames"].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in s._lib.mtgpu_last_error().decode()
    assert all(int((t != JUNK).sum()) == 0 for t in outs.values())


def test_motion_scores_unaligned_base(gpu_scanner_factory):
    """Integer-valued terms (every sum exact in any order, so the lanes a record falls to cannot change a bit): scores
    and term counts bit-equal to the CPU sum at byte shifts 4, 12, 20."""
    import torch
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    mv, off = ms.integer_frames(np.random.RandomState(2), ms.SIZES)
    want, want_t = ms.oracle_scores(mv, off), ms.count_terms(mv, off)
    assert want.max() < 2 ** 53 and (want == np.floor(want)).all()
    raw = torch.from_numpy(np.ascontiguousarray(mv, dtype=m.MV_DTYPE).view(np.uint8).reshape(-1).copy())
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    n = len(off) - 1
    for shift in dei.UNALIGNED_SHIFTS:
        sc = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        tm = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
        s.motion_scores_device(shifted(raw, shift), d_off, scores=sc, terms=tm)
        torch.cuda.synchronize()
        assert np.array_equal(ms.bits(sc.cpu().numpy()), ms.bits(want)), shift
        assert np.array_equal(tm.cpu().numpy().view(np.uint32), want_t), shift
    sc = torch.full((n,), 9.0, dtype=torch.float64, device="cuda")
    tm = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    odd = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")[1:1 + raw.numel()]
    rc = s._lib.mtgpu_motion_scores_device(s._ctx, odd.data_ptr(), len(mv), d_off.data_ptr(), n, sc.data_ptr(), tm.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in s._lib.mtgpu_last_error().decode()
    assert sc.cpu().tolist() == [9.0] * n and tm.cpu().tolist() == [JUNK] * n


# ------------------------------------------------------------------ F. the 16-bit accumulator boundary

def test_activity_16_bit_accumulators_at_65535_frames(gpu_scanner_factory):
    """1080p defaults: 16-bit LDS accumulators, max_run 65 535.  One stream of 70 000 frames, each with two votes into
    cells (40, 30) and (41, 30): whatever run_frames asks for (the largest uint32 too), a workgroup flushes before a field passes 0xFFFF — the
    two cells read 70 000 and every other cell 0 (a carry out of a field lands in the neighbouring cell's).  Then two
    streams split at frame 65 535: a field that holds exactly 0xFFFF.  All values by hand."""
    p = m.ScanParams.from_config(1920, 1080)
    plan = m.activity_preview(p)
    assert plan["acc_bits"] == 16 and plan["max_run"] == 65535 == dei.ACC_SPLIT
    mv, off, sd = dei.acc_batch()
    s = gpu_scanner_factory(p)
    one = dei.acc_hand([dei.ACC_FRAMES])
    two = dei.acc_hand([dei.ACC_SPLIT, dei.ACC_FRAMES - dei.ACC_SPLIT])
    assert one[2].tolist() == [70000] and two[2].tolist() == [65535, 4465]
    for compact in (True, False):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for run in (10 ** 9, 65535, 0, 2 ** 32 - 1) if compact else (10 ** 9,):
            got = device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, dei.ACC_FRAMES]), compact, run_frames=run)
            assert_maps_equal(got, one, f"one stream, compact {compact}, run_frames {run}")
        got = device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, dei.ACC_SPLIT, dei.ACC_FRAMES]), compact, run_frames=10 ** 9)
        assert_maps_equal(got, two, f"two streams, compact {compact}")
    assert_maps_equal(s.activity_map(m.FrameBatch(mv, off, None, sd), [0, dei.ACC_SPLIT, dei.ACC_FRAMES]), two, "host entry")


# ------------------------------------------------------------------ G. the hand-derived check_frame goldens

@pytest.mark.parametrize("name,kw,case", load_hand_cases()[1], ids=id_of)
def test_hand_cases_through_sweep_and_activity_map(gpu_scanner_factory, name, kw, case):
    """Every hand-derived known answer of tests/golden/check_frame_hand_cases.json (the only expected values that do not
    come from the oracle) as the middle setting of a 3 x 3 sweep [+inf, T, 0] x [255, V, 0], and as the centre sum of
    the activity map of a context created with the case's own parameters."""
    p = m.ScanParams.from_config(**kw)
    assert (p.grid_w, p.grid_h) == (10, 10)
    mv, off, sd, hand = dei.hand_case_batch(case)
    thr, vec = dei.hand_case_settings(kw)
    rest = {k: v for k, v in kw.items() if k not in ("width", "height", "mv_threshold_sq", "vectors_needed")}
    want = oracle_sweep(kw["width"], kw["height"], rest, mv, off, sd, thr, vec)
    assert int(want[1, 1, 0]) == hand
    s = gpu_scanner_factory(p)
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, name)
    maps = model_maps(p, mv, off, sd, [0, 1], 0)
    got = s.activity_map(m.FrameBatch(mv, off, None, sd), [0, 1])
    assert int(got[1].sum()) == hand and got[2].tolist() == [int(sd[0])], name
    assert_maps_parity(s, mv, off, sd, [0, 1], maps[:3], name, host=False)


@pytest.mark.parametrize("name,kw,case", load_hand_cases()[1], ids=id_of)
def test_hand_cases_through_direction_and_plane_scans(gpu_scanner_factory, name, kw, case):
    """The same hand-derived answers through the direction scan with every sector allowed and through the plane scan
    with a plane of 0xFF, in a context created with the case's own parameters: centre count and flag by hand, on both
    record layouts."""
    from test_gpu_dir import device_dir
    from test_gpu_lanes import device_lanes
    p = m.ScanParams.from_config(**kw)
    mv, off, sd, hand = dei.hand_case_batch(case)
    flag = int(case["expect"]) if sd[0] else 0
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        fl, ce, _ = device_dir(s, d_rec, d_off, d_sd, compact, allow=0xFF)
        assert (ce.tolist(), fl.tolist()) == ([hand], [flag]), (name, "direction scan", compact)
        fl, ce, _ = device_lanes(s, d_rec, d_off, d_sd, compact, np.full((p.grid_h, p.grid_w), 0xFF, dtype=np.uint8))
        assert (ce.tolist(), fl.tolist()) == ([hand], [flag]), (name, "plane scan", compact)


def test_hand_cases_one_batch_through_sweep_and_activity_map(gpu_scanner_factory):
    """The cases that share the base parameters as ONE batch, one stream per frame: the centre plane of stream i sums
    to case i's hand value."""
    base, mv, off, sd, hand = dei.hand_base_batch()
    p = m.ScanParams.from_config(**base)
    thr, vec = dei.hand_case_settings(base)
    rest = {k: v for k, v in base.items() if k not in ("width", "height", "mv_threshold_sq", "vectors_needed")}
    want = oracle_sweep(base["width"], base["height"], rest, mv, off, sd, thr, vec)
    assert want[1, 1].tolist() == hand
    s = gpu_scanner_factory(p)
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, "base cases in one batch")
    soff = np.arange(len(hand) + 1, dtype=np.uint64)
    maps = model_maps(p, mv, off, sd, soff, 0)
    assert [int(maps[1][i].sum()) for i in range(len(hand))] == hand and maps[2].tolist() == sd.tolist()
    assert_maps_parity(s, mv, off, sd, soff, maps[:3], "base cases in one batch", runs=(0, 1, 4))
