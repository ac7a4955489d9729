"""GPU tier (`-m gpu`): one scan of the records for a grid of (MV_THRESHOLD_SQ, VECTORS_NEEDED) settings
(include/mtgpu_sweep.h, csrc/sweep_kernels.hip).  The expected counts of setting (T, V) are the oracle's
scan_centres with params_from_config(..., mv_threshold_sq=T, vectors_needed=V); every comparison is exact (integers,
bit patterns of doubles).  Outputs are pre-filled with junk: every element must be written by the call."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, synth

import oracle_binding as ob
from scan_checks import assert_counts_equal, cells_frame, device_centres_of, junk_padding, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = -7


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_sweep(width, height, kw, mv, off, sd, thresholds, vectors):
    """uint32 [T, V, F]: one oracle pass per setting."""
    out = np.zeros((len(thresholds), len(vectors), len(off) - 1), dtype=np.uint32)
    for t, thr in enumerate(thresholds):
        for v, vec in enumerate(vectors):
            p = ob.params_from_config(width, height, mv_threshold_sq=thr, vectors_needed=vec, **kw)
            out[t, v] = ob.scan_centres(p, mv, off, sd, nthreads=4)[1]
    return out


def junk_out(n_thr, n_vec, n_frames):
    import torch
    return torch.full((n_thr, n_vec, n_frames), JUNK, dtype=torch.int32, device="cuda")


def device_sweep(s, d_rec, d_off, d_sd, thresholds, vectors, compact, stream=None):
    """Through mtgpu_scan_sweep_device into a junk-filled block -> uint32 [T, V, F] on the host."""
    import torch
    out = junk_out(len(thresholds), len(vectors), d_off.numel() - 1)
    got = s.sweep_centres_device(d_rec, d_off, d_sd, thresholds, vectors, compact=compact, out=out, stream=stream)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy().view(np.uint32)


def assert_sweep_parity(s, mv, off, sd, thresholds, vectors, want, what):
    """The host entry and the device entry on 40-byte and on compact records, against `want` [T, V, F]."""
    got = s.sweep_centres(m.FrameBatch(mv, off, None, sd), thresholds, vectors)
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert_counts_equal(got.reshape(-1), want.reshape(-1), what + " host entry")
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        got = device_sweep(s, d_rec, d_off, d_sd, thresholds, vectors, compact)
        assert_counts_equal(got.reshape(-1), want.reshape(-1), what + (" device entry, compact" if compact else " device entry, 40-byte"))


T1, V1 = [1, 4, 16, 50], [1, 2, 4, 8]


@functools.lru_cache(maxsize=None)
def parity_input():
    """The input of test 1 (shared, read-only): (mv, off, sd, oracle counts [4, 4, 16])."""
    rng = np.random.RandomState(11)
    mv, off, sd = synth.random_frames(rng, 16, 3000, 1920, 1080)
    junk_padding(mv, rng)
    want = oracle_sweep(1920, 1080, {}, mv, off, sd, T1, V1)
    for a in (mv, off, sd, want):
        a.setflags(write=False)
    return mv, off, sd, want


# ------------------------------------------------------------------ 1. parity, every setting distinct

def test_parity_every_setting_distinct(gpu_scanner_factory):
    """1920x1080 defaults, 16 random frames, thresholds [1, 4, 16, 50] x vectors [1, 2, 4, 8]: all 16 x 16 counts equal
    the oracle's through the host entry and the device entry on both record forms.  The oracle's 16 count vectors are
    pairwise different (maximum count 743): a kernel that ignores a setting cannot pass.  The context's own settings
    play no part: a context created with other ones returns the same block."""
    mv, off, sd, want = parity_input()
    assert len({want[t, v].tobytes() for t in range(4) for v in range(4)}) == 16 and int(want.max()) == 743
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    assert_sweep_parity(s, mv, off, sd, T1, V1, want, "1080p 4x4")
    other = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, mv_threshold_sq=1e9, vectors_needed=200, clusters_needed=77))
    got = other.sweep_centres(m.FrameBatch(mv, off, None, sd), T1, V1)
    assert np.array_equal(got, want)


def test_profiled_sweep_records_one_triple_per_call(gpu_scanner_factory):
    """mtgpu_profile_enable: a sweep call is one profiled launch (all its passes count as scan time), with the same
    results."""
    mv, off, sd, want = parity_input()
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_sweep(s, d_rec, d_off, d_sd, T1 + T1, V1, False)        # eight thresholds: two passes
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert np.array_equal(got[:4], want) and np.array_equal(got[4:], want)


# ------------------------------------------------------------------ 2. order, duplicates, specials, two passes

def test_callers_order_duplicates_specials_two_passes(gpu_scanner_factory):
    """Thresholds [nan, 24.5, 25.0, inf, -1.0, 25.0] (NaN and <= 0 keep everything, +inf nothing, 24.5 == 25.0 on integer
    |d|^2; six tiles: two passes of three on 1080p, where five fit) x vectors [0, 1, 255, 259] (0: every cell active, 259 wraps
    to 3), 24 random frames and one frame with side data but no records (level 0 counts on its empty grid)."""
    thr = [float("nan"), 24.5, 25.0, float("inf"), -1.0, 25.0]
    vec = [0, 1, 255, 259]
    assert m.sweep_preview(m.ScanParams.from_config(1920, 1080), len(thr), len(vec))["passes"] == 2
    rng = np.random.RandomState(12)
    mv, off, sd = synth.random_frames(rng, 24, 3000, 1920, 1080)
    junk_padding(mv, rng)
    off = np.concatenate([off, off[-1:]]).astype(np.uint64)
    sd = np.concatenate([sd, [1]]).astype(np.uint8)
    want = oracle_sweep(1920, 1080, {}, mv, off, sd, thr, vec)
    assert np.array_equal(want[0], want[4]) and np.array_equal(want[2], want[5]) and np.array_equal(want[1], want[2])
    assert int(want[3, 1:].max()) == 0 and int(want[0, 1].max()) > int(want[2, 1].max()) > 0
    assert want[3, 0, 24] > 0 and want[0, 1, 24] == 0            # the empty frame: level 0 counts, level 1 does not
    assert not np.array_equal(want[0, 3], want[0, 1]) and int(want[0, 3].max()) > 0
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, "specials")


# ------------------------------------------------------------------ 3. the existing path at 4K

def test_agrees_with_the_existing_scan_at_4k(gpu_scanner_factory):
    """3840x2160 defaults (one tile per pass), 6 random frames of up to 20 000 records, [4, 16] x [2, 4]: each setting's
    slice equals mtgpu_scan_centres_device of a context created with that setting, and the oracle."""
    thr, vec = [4, 16], [2, 4]
    rng = np.random.RandomState(13)
    mv, off, sd = synth.random_frames(rng, 6, 20000, 3840, 2160)
    junk_padding(mv, rng)
    want = oracle_sweep(3840, 2160, {}, mv, off, sd, thr, vec)
    assert len({want[t, v].tobytes() for t in range(2) for v in range(2)}) == 4
    s = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160))
    assert m.sweep_preview(s.params, 2, 2)["thresholds_per_pass"] == 1
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, "4K 2x2")
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    got = device_sweep(s, d_rec, d_off, d_sd, thr, vec, True)
    for t, T in enumerate(thr):
        for v, V in enumerate(vec):
            one = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, mv_threshold_sq=T, vectors_needed=V))
            _, ce = device_centres_of(one, d_rec, d_off, d_sd, True)
            assert_counts_equal(got[t, v], ce, f"4K slice ({T}, {V}) against mtgpu_scan_centres_device")


# ------------------------------------------------------------------ 4. pile-up

def _spread(n, mags):
    """n (dx, dy) pairs cycling through the given |d|^2 values."""
    table = {2: (1, 1), 10: (3, 1), 29: (5, 2), 61: (6, 5)}
    return np.array([table[mags[i % len(mags)]] for i in range(n)], dtype=np.int64)


def _pile(cell_votes):
    """cell_votes: [(gx, gy, n, mags)] -> records into 16-pixel cells, |d|^2 cycling through mags."""
    parts = []
    for gx, gy, n, mags in cell_votes:
        mv = cells_frame([(gx * 16 + 8, gy * 16 + 8, n)])
        d = _spread(n, mags)
        mv["src_x"], mv["src_y"] = mv["dst_x"] - d[:, 0], mv["dst_y"] - d[:, 1]
        parts.append(mv)
    return np.concatenate(parts)


def test_pile_up_beyond_16_bits(gpu_scanner_factory):
    """Counters must be exact past 65 535 votes.  1920x1080 defaults: 120 x 68 cells, margin 3, centre rows 3 .. 64.
    |d|^2 cycles through 2, 10, 29 and 61 — one value in each bucket of the thresholds [1, 4, 16, 50]: [1, 4), [4, 16),
    [16, 50), [50, ..) — so a cell with n records holds n, 3n/4, n/2 and n/4 votes at the four thresholds.  (30 and 60,
    the values one would write down first, are not sums of two squares.)
      frame 0: 70 000 records into cell (40, 30), 66 000 into its right neighbour (41, 30).  The fewest votes any
               setting sees are 16 500 >= 255: both cells are active at every threshold and level, each has the other
               as an active neighbour, nothing else votes: 2 centres in all 8 settings.
      frame 1: cell (60, 20) holds 300 records of |d|^2 = 61; its neighbour (61, 20) holds 254 of |d|^2 = 61 and 5 of
               |d|^2 = 29.  Threshold 50: 300 and 254 votes — at level 255 only one cell is active, and a lone cell is
               no centre: 0; at level 1 both: 2.  Thresholds 1, 4, 16: 300 and 259: 2 at both levels."""
    thr, vec = [1, 4, 16, 50], [1, 255]
    f0 = _pile([(40, 30, 70000, (2, 10, 29, 61)), (41, 30, 66000, (2, 10, 29, 61))])
    f1 = _pile([(60, 20, 300, (61,)), (61, 20, 254, (61,)), (61, 20, 5, (29,))])
    rng = np.random.RandomState(14)
    frames = [f0[rng.permutation(len(f0))], f1[rng.permutation(len(f1))]]
    b = m.FrameBatch.from_frames(frames)
    hand = np.full((4, 2, 2), 2, dtype=np.uint32)
    hand[3, 1, 1] = 0
    want = oracle_sweep(1920, 1080, {}, b.mv, b.frame_off, b.has_sd, thr, vec)
    assert np.array_equal(want, hand)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    assert_sweep_parity(s, b.mv, b.frame_off, b.has_sd, thr, vec, hand, "pile-up")


# ------------------------------------------------------------------ 5. widths and edges

@pytest.mark.parametrize("width,height", [(1008, 64), (1024, 64), (1040, 64), (2064, 96)])
def test_grid_widths_around_the_mask_word(gpu_scanner_factory, width, height):
    """vertical_mask = 0 (the grid's first and last row are centres) on grids 63, 64, 65 and 129 cells wide: neighbours
    across the 64-bit word boundary, the last column never a centre."""
    thr, vec = [4, 16], [1, 2, 3]
    rng = np.random.RandomState(width)
    mv, off, sd = synth.random_frames(rng, 12, 3000, width, height)
    junk_padding(mv, rng)
    kw = dict(vertical_mask=0.0)
    want = oracle_sweep(width, height, kw, mv, off, sd, thr, vec)
    assert int(want.max()) > 0 and len({want[t, v].tobytes() for t in range(2) for v in range(3)}) == 6
    s = gpu_scanner_factory(m.ScanParams.from_config(width, height, **kw))
    assert s.params.grid_w == (width + 15) // 16 and s.params.vertical_margin == 0
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, f"{width}x{height}")


def test_edges_one_column_no_side_data_no_frames_windows(gpu_scanner_factory):
    import torch
    lib = m.load_library()
    thr, vec = [4, 16], [0, 1, 2]
    # a grid one cell wide: no column in [1, gw - 2], whatever the level
    rng = np.random.RandomState(15)
    mv, off, sd = synth.random_frames(rng, 12, 500, 16, 16)
    s1 = gpu_scanner_factory(m.ScanParams.from_config(16, 16, vertical_mask=0.0))
    assert s1.params.grid_w == 1
    want = oracle_sweep(16, 16, dict(vertical_mask=0.0), mv, off, sd, thr, vec)
    assert int(want.max()) == 0
    assert_sweep_parity(s1, mv, off, sd, thr, vec, want, "16x16")

    # frames without side data: 0 in every setting, level 0 included, also when they own records
    rng = np.random.RandomState(16)
    mv, off, sd = synth.random_frames(rng, 20, 3000, 1920, 1080)
    sd = sd.copy()
    sd[[2, 5, 11]] = 0
    assert int(off[3]) > int(off[2])
    want = oracle_sweep(1920, 1080, {}, mv, off, sd, thr, vec)
    assert int(want[:, :, sd == 0].max()) == 0 and int(want[:, 0, sd != 0].min()) > 0
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    assert_sweep_parity(s, mv, off, sd, thr, vec, want, "no side data")
    # has_sd == NULL: side data iff records
    want_nosd = oracle_sweep(1920, 1080, {}, mv, off, None, thr, vec)
    assert_sweep_parity(s, mv, off, None, thr, vec, want_nosd, "has_sd NULL")

    # n_frames == 0: MT_OK, nothing written
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    out = junk_out(2, 3, 4)
    c_thr, c_vec = (C.c_double * 2)(*thr), (C.c_int32 * 3)(*vec)
    assert lib.mtgpu_scan_sweep_device(s._ctx, d_rec.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), 0, c_thr, 2,
                                       c_vec, 3, out.data_ptr(), None) == _abi.MT_OK
    torch.cuda.synchronize()
    assert int((out != JUNK).sum()) == 0
    assert s.sweep_centres(m.FrameBatch(mv[:0], off[:1], None, None), thr, vec).shape == (2, 3, 0)

    # offsets that are a window of a larger batch: frames 6 .. 15
    a, b = 6, 16
    assert int(off[a]) > 0
    got = s.sweep_centres(m.FrameBatch(mv, off[a:b + 1], None, sd[a:b]), thr, vec)
    assert_counts_equal(got.reshape(-1), want[:, :, a:b].reshape(-1), "window, host entry")
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        got = device_sweep(s, d_rec, d_off[a:b + 1], d_sd[a:b], thr, vec, compact)
        assert_counts_equal(got.reshape(-1), want[:, :, a:b].reshape(-1), "window, device entry")


# ------------------------------------------------------------------ 6. unsupported and invalid

def test_unsupported_grid_and_invalid_arguments_launch_nothing(gpu_scanner_factory):
    import torch
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    rec = torch.zeros(8 * 16 + 8, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device="cuda")
    out = junk_out(8, 8, 2)
    thr, vec = (C.c_double * 9)(*range(1, 10)), (C.c_int32 * 9)(*range(1, 10))

    def err():
        return lib.mtgpu_last_error().decode()

    def call(s, rec_ptr=None, rb=8, t=thr, nt=2, v=vec, nv=2, o=out.data_ptr()):
        return lib.mtgpu_scan_sweep_device(s._ctx, rec.data_ptr() if rec_ptr is None else rec_ptr, rb, 8, off.data_ptr(), None,
                                           2, t, nt, v, nv, o, None)

    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert (big.params.grid_w, big.params.grid_h) == (960, 540)
    assert call(big) == _abi.MT_ERR_UNSUPPORTED and "960x540" in err()
    with pytest.raises(m.MtgpuError) as ei:
        big.sweep_centres(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)), [4], [2])
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)

    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    for rb in (0, 7, 16, 39, 41, -8):
        assert call(s, rb=rb) == inv and "rec_bytes" in err()
    assert call(s, rec_ptr=rec.data_ptr() + 4) == inv and "d_rec" in err() and "8-byte" in err()
    assert call(s, t=None) == inv and "thresholds" in err()
    assert call(s, v=None) == inv and "vectors" in err()
    assert call(s, o=None) == inv and "d_centres" in err()
    for n in (0, 9):
        assert call(s, nt=n) == inv and "n_thresholds" in err()
        assert call(s, nv=n) == inv and "n_vectors" in err()
    assert lib.mtgpu_scan_frames_sweep(s._ctx, None, None, None, 2, thr, 2, vec, 2, None) == inv
    assert lib.mtgpu_scan_frames_sweep(s._ctx, None, None, None, 2, thr, 9, vec, 2, None) == inv and "n_thresholds" in err()
    torch.cuda.synchronize()
    assert int((out != JUNK).sum()) == 0            # nothing was launched: no output word changed
    assert call(s) == _abi.MT_OK                      # and the same call with valid arguments runs
    torch.cuda.synchronize()
    assert int((out.reshape(-1)[:8] != JUNK).sum()) == 8 and int((out.reshape(-1)[8:] != JUNK).sum()) == 0


# ------------------------------------------------------------------ 7. exact extent

def test_exactly_the_block_is_written():
    """d_centres as a view into a larger junk tensor, in device memory and in pinned host memory (system-scope
    stores): T x V x F words hold the counts, the words before and behind are unchanged."""
    import torch
    mv, off, sd, want = parity_input()
    n = want.size
    with m.MotionScanner(m.ScanParams.from_config(1920, 1080)) as s:
        d_rec, d_off, d_sd = to_device(mv, off, sd, True)
        dev = torch.full((n + 96,), JUNK, dtype=torch.int32, device="cuda")
        pinned = torch.full((n + 96,), JUNK, dtype=torch.int32).pin_memory()
        for buf in (dev, pinned):
            view = buf[32:32 + n].view(4, 4, 16)
            c_thr, c_vec = (C.c_double * 4)(*T1), (C.c_int32 * 4)(*V1)
            _abi.check(s._lib.mtgpu_scan_sweep_device(s._ctx, d_rec.data_ptr(), 8, len(mv), d_off.data_ptr(), d_sd.data_ptr(),
                                                      16, c_thr, 4, c_vec, 4, view.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            raw = buf.cpu().numpy()
            assert np.array_equal(raw[32:32 + n].view(np.uint32).reshape(want.shape), want)
            assert (raw[:32] == JUNK).all() and (raw[32 + n:] == JUNK).all()


# ------------------------------------------------------------------ 8. two streams at once

def test_two_threads_on_their_own_streams(gpu_scanner_factory):
    import torch
    mv, off, sd, want = parity_input()
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    d40 = to_device(mv, off, sd, False)
    d8 = to_device(mv, off, sd, True)
    torch.cuda.synchronize()
    results, errors = [[], []], []

    def work(i):
        try:
            st = torch.cuda.Stream()
            d_rec, d_off, d_sd = d8 if i else d40
            outs = [junk_out(4, 4, 16) for _ in range(4)]
            torch.cuda.synchronize()                  # the junk fill ran on torch's stream, the calls run on `st`
            for out in outs:
                s.sweep_centres_device(d_rec, d_off, d_sd, T1, V1, compact=bool(i), out=out, stream=st.cuda_stream)
                results[i].append(out)
            st.synchronize()
        except Exception as e:                        # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert len(results[i]) == 4
        for out in results[i]:
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want), i


# ------------------------------------------------------------------ 9. end to end

def test_end_to_end_study_and_command(gpu_scanner_factory, tmp_path):
    """2 streams x 96 frames of spec_1080p(sub=1) with scripted events, [4, 16] x [2, 4] x clusters [1, 2, 4]: the
    sweep, then sweep_streams_device per pair — segments and mt_merge_result bit-equal to the oracle's pool_and_merge of
    the pts of the frames the oracle flags with each (T, V, C).  `python -m mvtrim_amd.tune --json` on the first stream
    written as .mtmv prints the same rows.  (event_records=3: with sub=1 a cell holds one record, which no VECTORS_NEEDED
    >= 2 can make active; three records per cell of a moving region let level 2 say yes and level 4 say no.)"""
    import torch
    from mvtrim_amd import tune
    thr, vec, clu = [4, 16], [2, 4], [1, 2, 4]
    S, F, CAP = 2, 96, 32
    parts, paths = [], []
    for i in range(S):
        spec = synth.spec_1080p(seed=31 + i, sub=1, event_records=3)
        spec.events = synth.scripted_events(spec, F)
        frames = [synth.gen_frame(spec, f) for f in range(F)]
        path = str(tmp_path / f"stream{i}.mtmv")
        m.mvfile.write_mtmv(path, spec.width, spec.height, 1, spec.tb_den, spec.fps, F / spec.fps,
                            [spec.pts_ticks(f) for f in range(F)], frames)
        batch, pts, hdr = tune.load(path)             # the seconds the command works with
        assert batch.n_frames == F and hdr["width"] == 1920 and hdr["duration"] == F / spec.fps
        parts.append((batch, pts))
        paths.append(path)
    mv = np.concatenate([b.mv for b, _ in parts])
    off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b.frame_off.astype(np.int64)) for b, _ in parts]))]).astype(np.uint64)
    sd = np.concatenate([b.has_sd for b, _ in parts])
    pts = np.concatenate([p for _, p in parts])
    mps = [m.MergeParams(duration=F / 30.0, max_gap_sec=0.2, padding_sec=0.05, min_savings_pct=5.0) for _ in range(S)]
    want = oracle_sweep(1920, 1080, {}, mv, off, sd, thr, vec)
    assert len({(want[t, v] >= c).tobytes() for t in range(2) for v in range(2) for c in clu}) >= 2

    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    d_pts = torch.from_numpy(pts).cuda()
    soff = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * F).cuda()
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    centres = s.sweep_centres_device(d_rec, d_off, d_sd, thr, vec, out=junk_out(2, 2, S * F))
    rows0 = []
    for t, T in enumerate(thr):
        for v, V in enumerate(vec):
            seg, res = s.sweep_streams_device(centres[t, v], d_pts, soff, d_mp, clu, seg_cap=CAP)
            torch.cuda.synchronize()
            seg_h, res_h = seg.cpu().numpy(), res.cpu().numpy()
            for ci, c in enumerate(clu):
                p = ob.params_from_config(1920, 1080, mv_threshold_sq=T, vectors_needed=V, clusters_needed=c)
                flags = ob.scan_frames(p, mv, off, sd, nthreads=4)
                assert np.array_equal(flags, (want[t, v] >= c).astype(np.uint8))
                recs = m.results_from_bytes(res_h[ci])
                for i in range(S):
                    a, b = i * F, (i + 1) * F
                    wseg, wres = ob.pool_and_merge(pts[a:b][flags[a:b] != 0], mps[i], False)
                    wrec = np.zeros(1, dtype=m.MERGE_RESULT_DTYPE)
                    for k, val in wres.items():
                        wrec[k] = val
                    assert recs[i:i + 1].tobytes() == wrec.tobytes(), (T, V, c, i, recs[i], wres)
                    k = int(wres["n_segments"])
                    assert np.array_equal(bits(seg_h[ci, i, :k, 0]), bits(wseg["start"])), (T, V, c, i)
                    assert np.array_equal(bits(seg_h[ci, i, :k, 1]), bits(wseg["end"])), (T, V, c, i)
                    if i == 0:
                        rows0.append({"mv_threshold_sq": float(T), "vectors_needed": V, "clusters_needed": c,
                                      "motion_frames": int(wres["n_timestamps"]), "segments": k,
                                      "saved_pct": float(wres["saved_pct"]), "do_cut": int(wres["do_cut"])})
    assert any(r["segments"] > 0 and r["do_cut"] == 1 for r in rows0) and any(r["motion_frames"] == 0 for r in rows0)

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.tune", paths[0], "--mv-threshold-sq", "4,16", "--vectors-needed",
                          "2,4", "--clusters-needed", "1,2,4", "--max-gap-sec", "0.2", "--padding-sec", "0.05",
                          "--min-savings-pct", "5", "--json"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert doc["width"] == 1920 and doc["height"] == 1080 and doc["frames"] == F
    assert doc["rows"] == rows0
