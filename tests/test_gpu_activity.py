"""GPU tier (`-m gpu`): per-stream activity maps (include/mtgpu_activity.h, csrc/activity_kernels.hip).

The per-cell expectation is the numpy model of tests/activity_model.py (histogram, saturate at 255, `>= vn`, shifted
planes — the style of np_model.check_frame_np, which it extends by vn == 0 with a margin, analysed-rows-only for the
active plane and contribution by min_centres).  Two identities tie the model to the oracle in every parity check: per stream,
centre.sum() == the sum of the oracle's centre counts over the contributing frames, and frames[s] == the number of
frames with side data whose oracle count is >= min_centres.  Every comparison is exact; outputs are pre-filled with
junk: every element must be written by the call."""
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
from mvtrim_amd import _abi, config, synth

import oracle_binding as ob
from activity_model import assert_oracle_identities, frame_planes, model_maps    # noqa: F401 (re-exported)
from scan_checks import cells_frame, device_centres_of, junk_padding, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = -7
PARAM_SETS = (config.CODE_DEFAULTS, config.SHIPPED_ENV)


# ------------------------------------------------------------------ device helpers

def soff_tensor(stream_off):
    import torch
    return torch.from_numpy(np.asarray(stream_off).astype(np.int64)).cuda()


def junk_maps(s, n_streams, want=("active", "centre", "frames")):
    import torch
    gh, gw = s.params.grid_h, s.params.grid_w
    return {n: torch.full((n_streams,) if n == "frames" else (n_streams, gh, gw), JUNK, dtype=torch.int32, device="cuda")
            for n in want}


def device_maps(s, d_rec, d_off, d_sd, d_soff, compact, min_centres=0, run_frames=0, want=("active", "centre", "frames"),
                stream=None):
    """Through mtgpu_activity_map_device into junk-filled outputs -> numpy uint32 arrays (None where not wanted)."""
    import torch
    out = junk_maps(s, d_soff.numel() - 1, want)
    torch.cuda.synchronize()
    got = s.activity_map_device(d_rec, d_off, d_sd, d_soff, min_centres=min_centres, run_frames=run_frames, want=want,
                                compact=compact, out=out, stream=stream)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy().view(np.uint32) for t in got)


def assert_maps_equal(got, want, what):
    for name, g, w in zip(("active", "centre", "frames"), got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (f"{what}: {name} differs in {len(bad)} of {w.size} elements, first {bad[:6].tolist()}: "
                               f"want {[int(w[tuple(i)]) for i in bad[:6]]} got {[int(g[tuple(i)]) for i in bad[:6]]}")


# ------------------------------------------------------------------ the inputs (shared, read-only)

STREAMS_1 = np.array([0, 1, 38, 128], dtype=np.uint64)               # three streams of 1, 37 and 90 frames


@functools.lru_cache(maxsize=None)
def parity_input():
    """128 ragged random 1080p frames: records outside the grid and in masked rows, every 5th frame without side data,
    some frames with side data and no record."""
    rng = np.random.RandomState(21)
    mv, off, sd = synth.random_frames(rng, 128, 3000, 1920, 1080)
    # random cells rarely fill an edge column: frames 7, 21 and 77 get two pairs of cells that do (5 and 6 votes each)
    parts = [mv[int(off[f]):int(off[f + 1])] for f in range(128)]
    for f in (7, 21, 77):
        edge = cells_frame([(3, 10 * 16, 5), (19, 10 * 16 + f % 16, 5), (119 * 16 + 2, 40 * 16, 6), (118 * 16, 40 * 16 + 9, 6)])
        edge["w"], edge["h"], edge["source"], edge["motion_scale"] = 8, 8, -1, 4
        both = np.zeros(len(parts[f]) + len(edge), dtype=m.MV_DTYPE)
        both[:len(parts[f])], both[len(parts[f]):] = parts[f], edge
        parts[f] = both[rng.permutation(len(both))]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
    mv = np.zeros(int(off[-1]), dtype=m.MV_DTYPE)
    for f in range(128):
        mv[int(off[f]):int(off[f + 1])] = parts[f]
    junk_padding(mv, rng)
    sd = sd.copy()
    sd[::5] = 0
    sd[[7, 21, 77]] = 1
    empty = np.diff(off.astype(np.int64)) == 0
    assert int((empty & (sd != 0)).sum()) >= 3 and int(((~empty) & (sd == 0)).sum()) >= 3
    for a in (mv, off, sd):
        a.setflags(write=False)
    return mv, off, sd


@functools.lru_cache(maxsize=None)
def parity_model(which, min_centres):
    """The model's maps of parity_input under PARAM_SETS[which], checked against the oracle's counts."""
    mv, off, sd = parity_input()
    p = m.ScanParams.from_config(1920, 1080, **PARAM_SETS[which])
    want = model_maps(p, mv, off, sd, STREAMS_1, min_centres)
    assert_oracle_identities(p, mv, off, sd, STREAMS_1, min_centres, want[1], want[2], "model")
    for a in want:
        a.setflags(write=False)
    return p, want


N_BOUNDARY = 4096


@functools.lru_cache(maxsize=None)
def boundary_input():
    """4096 frames built cell by cell on the 1080p grid (120 x 68, margin 3): frame f holds a horizontal pair of cells
    with 2 + f % 3 and 2 + f % 2 votes (two centres under VECTORS_NEEDED 2), a lone 3-vote cell (active, no centre),
    a 1-vote cell (inactive) and a pair inside the masked rows (never counted).  Every 11th frame has no side data,
    every 13th has side data and no record."""
    frames, sd = [], []
    for f in range(N_BOUNDARY):
        x, y = 1 + (f * 7) % 110, 3 + (f * 5) % 62
        cells = [(x * 16 + 3, y * 16 + 5, 2 + f % 3), ((x + 1) * 16 + 9, y * 16 + 1, 2 + f % 2),
                 (((x + 40) % 118 + 1) * 16, ((y + 30) % 62 + 3) * 16, 3), (((x + 60) % 118 + 1) * 16, ((y + 9) % 62 + 3) * 16, 1),
                 (x * 16, 1 * 16, 4), ((x + 1) * 16, 1 * 16, 4)]
        frames.append(cells_frame(cells) if f % 13 else np.zeros(0, dtype=m.MV_DTYPE))
        sd.append(0 if f % 11 == 0 else 1)
    counts = np.array([len(x) for x in frames], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    mv = np.ascontiguousarray(np.concatenate(frames), dtype=m.MV_DTYPE)
    sd = np.array(sd, dtype=np.uint8)
    for a in (mv, off, sd):
        a.setflags(write=False)
    return mv, off, sd


STREAMS_7 = np.minimum(np.arange(587, dtype=np.uint64) * 7, N_BOUNDARY)      # 586 streams of 7 frames, the last shorter


@functools.lru_cache(maxsize=None)
def boundary_model():
    mv, off, sd = boundary_input()
    p = m.ScanParams.from_config(1920, 1080, **config.CODE_DEFAULTS)
    assert len(STREAMS_7) == 587 and int(STREAMS_7[-1]) == N_BOUNDARY and int(STREAMS_7[-1] - STREAMS_7[-2]) == 1
    many = model_maps(p, mv, off, sd, STREAMS_7, 0)
    assert_oracle_identities(p, mv, off, sd, STREAMS_7, 0, many[1], many[2], "model, 586 streams")
    one = (many[0].sum(axis=0, dtype=np.uint32)[None], many[1].sum(axis=0, dtype=np.uint32)[None],
           np.array([many[2].sum()], dtype=np.uint32))
    return p, many[:3], one


# ------------------------------------------------------------------ 1. per-cell parity

@pytest.mark.parametrize("which", [0, 1])
def test_per_cell_parity(gpu_scanner_factory, which):
    """1080p, code defaults / shipped env, three streams of 1, 37 and 90 ragged frames, both record layouts,
    run_frames 0, 1, 2, 3, 64: the maps equal the model's and each other's; the host entry point too."""
    mv, off, sd = parity_input()
    p, want = parity_model(which, 0)
    assert int(want[1].sum()) > 0 and int(want[0].sum()) > int(want[1].sum()) and want[2].tolist() != [0, 0, 0]
    s = gpu_scanner_factory(p)
    d_soff = soff_tensor(STREAMS_1)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for run in (0, 1, 2, 3, 64):
            got = device_maps(s, d_rec, d_off, d_sd, d_soff, compact, run_frames=run)
            assert_maps_equal(got, want[:3], f"set {which} compact {compact} run_frames {run}")
    got = s.activity_map(m.FrameBatch(mv, off, None, sd), STREAMS_1)
    assert_maps_equal(got, want[:3], "host entry")
    assert_oracle_identities(p, mv, off, sd, STREAMS_1, 0, got[1], got[2], "device")
    # has_sd == NULL: the scan's rule — side data iff records
    want_null = model_maps(p, mv, off, None, STREAMS_1, 0)
    d_rec, d_off, _ = to_device(mv, off, sd, True)
    assert_maps_equal(device_maps(s, d_rec, d_off, None, d_soff, True), want_null[:3], "has_sd NULL")
    assert_oracle_identities(p, mv, off, None, STREAMS_1, 0, want_null[1], want_null[2], "model, has_sd NULL")


# ------------------------------------------------------------------ 2. run and stream boundaries

def test_run_and_stream_boundaries(gpu_scanner_factory):
    """4096 cell-built frames.  586 streams of 7 frames with run_frames 0, 5, 7, 16: stream boundaries at the start, in
    the middle and at the end of runs.  One stream of all frames with run_frames = max_run (and 4096 where a 16-bit
    plan allows more): one workgroup collects everything."""
    mv, off, sd = boundary_input()
    p, many, one = boundary_model()
    assert int(many[1].sum()) > 0 and int(many[2].min()) >= 1
    s = gpu_scanner_factory(p)
    plan = m.activity_preview(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_soff = soff_tensor(STREAMS_7)
    for run in (0, 5, 7, 16):
        assert_maps_equal(device_maps(s, d_rec, d_off, d_sd, d_soff, True, run_frames=run), many, f"586 streams, run_frames {run}")
    d_one = soff_tensor([0, N_BOUNDARY])
    runs = [plan["max_run"]] + ([N_BOUNDARY] if plan["acc_bits"] == 16 and plan["max_run"] > N_BOUNDARY else [])
    for run in runs:
        assert_maps_equal(device_maps(s, d_rec, d_off, d_sd, d_one, True, run_frames=run), one, f"one stream, run_frames {run}")
    # empty streams between the others, and run_frames far above n_frames
    soff = np.array([0, 0, 7, 7, 7, 14, N_BOUNDARY, N_BOUNDARY], dtype=np.uint64)
    want = model_maps(p, mv, off, sd, soff, 0)[:3]
    for run in (0, 3, 10 ** 9):
        assert_maps_equal(device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), True, run_frames=run), want, f"empty streams, run_frames {run}")


# ------------------------------------------------------------------ 3. pile-up

def test_pile_up_beyond_16_bits(gpu_scanner_factory):
    """One frame, 70 000 kept records in cell (40, 30) and 70 000 in its neighbour (41, 30), VECTORS_NEEDED 255: both
    are active and centres, once; votes past 16 bits leak into no other cell."""
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=255)
    mv = cells_frame([(40 * 16 + 8, 30 * 16 + 8, 70000), (41 * 16 + 8, 30 * 16 + 8, 70000)])
    mv = mv[np.random.RandomState(3).permutation(len(mv))]
    off = np.array([0, len(mv)], dtype=np.uint64)
    sd = np.ones(1, dtype=np.uint8)
    hand = np.zeros((1, 68, 120), dtype=np.uint32)
    hand[0, 30, 40:42] = 1
    want = model_maps(p, mv, off, sd, [0, 1], 0)
    assert np.array_equal(want[0], hand) and np.array_equal(want[1], hand) and want[2].tolist() == [1]
    assert_oracle_identities(p, mv, off, sd, [0, 1], 0, want[1], want[2], "model")
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        assert_maps_equal(device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, 1]), compact), want[:3], f"pile-up compact {compact}")


# ------------------------------------------------------------------ 4. vectors_needed == 0

@pytest.mark.parametrize("mask,margin", [(0.0, 0), (0.05, 3)])
def test_vectors_needed_zero(gpu_scanner_factory, mask, margin):
    """Every analysed cell is active in every frame with side data, the frames with no record included; nothing is
    counted for a frame without side data; the centre plane follows the scan (masked neighbour rows count as active)."""
    mv, off, sd = parity_input()
    mv, off, sd = mv[:int(off[40])], off[:41], sd[:40]
    soff = np.array([0, 13, 40], dtype=np.uint64)
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=0, vertical_mask=mask)
    assert p.vertical_margin == margin and p.vectors_needed == 0
    s = gpu_scanner_factory(p)
    want = model_maps(p, mv, off, sd, soff, 0)
    assert_oracle_identities(p, mv, off, sd, soff, 0, want[1], want[2], "model")
    n_sd = np.array([int(sd[:13].sum()), int(sd[13:].sum())], dtype=np.uint32)
    assert np.array_equal(want[2], n_sd) and int(n_sd.min()) > 0 and int((sd == 0).sum()) > 0
    assert int(((np.diff(off.astype(np.int64)) == 0) & (sd != 0)).sum()) > 0
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), compact)
        assert_maps_equal(got, want[:3], f"vn 0 margin {margin} compact {compact}")
        for i in range(2):
            assert (got[0][i, margin:68 - margin, :] == n_sd[i]).all()
            assert int(got[0][i, :margin].sum()) == 0 and int(got[0][i, 68 - margin:].sum()) == 0
            assert (got[1][i, margin:68 - margin, 1:119] == n_sd[i]).all()          # every inner cell has an active neighbour
        _, ce = device_centres_of(s, d_rec, d_off, d_sd, compact)
        assert [int(got[1][i].sum()) for i in range(2)] == [int(ce[:13].sum()), int(ce[13:].sum())]
        assert int(ce[sd == 0].sum()) == 0


# ------------------------------------------------------------------ 5. min_centres

@pytest.mark.parametrize("min_centres", [0, 1, 2, 10 ** 9])
def test_min_centres(gpu_scanner_factory, min_centres):
    mv, off, sd = parity_input()
    p, want = parity_model(1, min_centres)
    counts = want[3]
    if min_centres == 10 ** 9:
        assert not want[0].any() and not want[1].any() and not want[2].any()
    elif min_centres:
        # the threshold separates frames: some with side data stay out (those without a record at least), some get in
        assert 0 < int(want[2].sum()) < int(parity_model(1, 0)[1][2].sum())
        assert int(want[2].sum()) == int(((counts >= min_centres) & (sd != 0)).sum())
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    for run in (0, 3):
        got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(STREAMS_1), True, min_centres=min_centres, run_frames=run)
        assert_maps_equal(got, want[:3], f"min_centres {min_centres} run_frames {run}")
    got = s.activity_map(m.FrameBatch(mv, off, None, sd), STREAMS_1, min_centres=min_centres)
    assert_maps_equal(got, want[:3], f"min_centres {min_centres} host entry")


# ------------------------------------------------------------------ 6. the direct form at 4K

@pytest.mark.parametrize("which", [0, 1])
def test_4k_direct_form(gpu_scanner_factory, which):
    """3840x2160 (240 x 135 cells, no room for accumulators): eight cell-built frames in two streams; per cell against
    the model, per frame against mtgpu_scan_centres_device."""
    p = m.ScanParams.from_config(3840, 2160, **PARAM_SETS[which])
    assert m.activity_preview(p)["acc_bits"] == 0 and (p.grid_w, p.grid_h) == (240, 135)
    frames = []
    for f in range(8):
        cells = []
        for j in range(40):                                    # blobs of 2 x 2 cells, 4 or 5 votes each, and lone cells
            x, y = 2 + (j * 37 + f * 11) % 230, 7 + (j * 23 + f * 5) % 118
            cells += [(x * 16 + 1, y * 16 + 2, 4 + j % 2), ((x + 1) * 16, y * 16, 5), (x * 16, (y + 1) * 16 + 7, 4),
                      (((x + 100) % 236 + 1) * 16, ((y + 50) % 118 + 7) * 16, 9)]
        cells += [(0, 60 * 16, 6), (16, 60 * 16, 6), (239 * 16, 70 * 16, 6), (238 * 16, 70 * 16, 6), (100 * 16, 2 * 16, 9)]
        frames.append(cells_frame(cells))
    frames[5] = np.zeros(0, dtype=m.MV_DTYPE)
    b = m.FrameBatch.from_frames(frames)
    mv, off = b.mv, b.frame_off
    sd = np.array([1, 1, 0, 1, 1, 1, 1, 1], dtype=np.uint8)
    soff = np.array([0, 3, 8], dtype=np.uint64)
    s = gpu_scanner_factory(p)
    for min_centres in (0, 1):
        want = model_maps(p, mv, off, sd, soff, min_centres)
        assert int(want[1].sum()) > 0 and want[2].tolist() == ([2, 5] if min_centres == 0 else [2, 4])
        assert int(want[0][:, :, 0].sum()) > 0 and int(want[0][:, :, 239].sum()) > 0 and int(want[1][:, :, [0, 239]].sum()) == 0
        assert_oracle_identities(p, mv, off, sd, soff, min_centres, want[1], want[2], "model")
        for compact in (False, True):
            d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
            for run in (0, 4):
                got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), compact, min_centres=min_centres, run_frames=run)
                assert_maps_equal(got, want[:3], f"4K set {which} min_centres {min_centres} compact {compact} run_frames {run}")
            _, ce = device_centres_of(s, d_rec, d_off, d_sd, compact)
            take = ce.astype(np.int64) >= min_centres
            assert [int(got[1][i].sum()) for i in range(2)] == [int(ce[:3][take[:3]].sum()), int(ce[3:][take[3:]].sum())]


# ------------------------------------------------------------------ 7. grid widths around the mask word

@pytest.mark.parametrize("width,gw", [(48, 3), (1008, 63), (1024, 64), (1040, 65), (2048, 128), (2064, 129)])
def test_grid_widths_around_the_mask_word(gpu_scanner_factory, width, gw):
    """vertical_mask 0 (the grid's first and last row are centres; the row outside the grid is inactive) on grids whose
    rows end before, at and behind a 64-bit mask word, and whose width is no multiple of the four-cell accumulator unit."""
    rng = np.random.RandomState(width)
    mv, off, sd = synth.random_frames(rng, 12, 3000, width, 64)
    junk_padding(mv, rng)
    p = m.ScanParams.from_config(width, 64, vertical_mask=0.0)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (gw, 4, 0)
    soff = np.array([0, 5, 12], dtype=np.uint64)
    want = model_maps(p, mv, off, sd, soff, 0)
    assert int(want[1].sum()) > 0 and int(want[0][:, :, gw - 1].sum()) > 0 and int(want[1][:, [0, 3]].sum()) > 0
    assert_oracle_identities(p, mv, off, sd, soff, 0, want[1], want[2], "model")
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for run in (0, 1, 5):
            got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), compact, run_frames=run)
            assert_maps_equal(got, want[:3], f"gw {gw} compact {compact} run_frames {run}")


def test_two_columns_and_empty_analysed_range(gpu_scanner_factory):
    rng = np.random.RandomState(7)
    # gw == 2: no column in [1, gw - 2] — no centres, the active cells are still counted
    mv, off, sd = synth.random_frames(rng, 12, 500, 32, 48)
    p = m.ScanParams.from_config(32, 48, vertical_mask=0.0, vectors_needed=1)
    assert p.grid_w == 2
    want = model_maps(p, mv, off, sd, [0, 12], 0)
    assert int(want[1].sum()) == 0 and int(want[0].sum()) > 0
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    assert_maps_equal(device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, 12]), False), want[:3], "gw 2")
    assert not device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, 12]), False, min_centres=1)[2].any()
    # margin >= gh / 2: nothing is analysed; with min_centres == 0 the frames still contribute
    mv, off, sd = synth.random_frames(rng, 12, 3000, 1920, 1080)
    p = m.ScanParams.from_config(1920, 1080, vertical_mask=0.5)
    assert 2 * p.vertical_margin >= p.grid_h
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    for run in (0, 5):
        a, c, f = device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, 4, 12]), True, run_frames=run)
        assert not a.any() and not c.any() and f.tolist() == [int(sd[:4].sum()), int(sd[4:].sum())] and int(f.sum()) > 0
    assert not device_maps(s, d_rec, d_off, d_sd, soff_tensor([0, 4, 12]), True, min_centres=1)[2].any()


# ------------------------------------------------------------------ 8. unsupported and invalid

def test_unsupported_grid_and_invalid_arguments_launch_nothing(gpu_scanner_factory):
    import torch
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    rec = torch.zeros(8 * 16 + 8, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device="cuda")
    soff = torch.tensor([0, 1, 2], dtype=torch.int64, device="cuda")
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    outs = junk_maps(s, 2)
    pinned = torch.full((2 * 68 * 120,), JUNK, dtype=torch.int32).pin_memory()

    def err():
        return lib.mtgpu_last_error().decode()

    def call(ctx, rec_ptr=None, rb=8, o=None, so=None, a="x", c="x", f="x"):
        ptr = lambda v, t: t.data_ptr() if v == "x" else v        # noqa: E731
        return lib.mtgpu_activity_map_device(ctx._ctx, rec.data_ptr() if rec_ptr is None else rec_ptr, rb, 8,
                                             off.data_ptr() if o is None else o, None, 2, soff.data_ptr() if so is None else so, 2,
                                             0, 0, ptr(a, outs["active"]), ptr(c, outs["centre"]), ptr(f, outs["frames"]), None)

    assert (big.params.grid_w, big.params.grid_h) == (960, 540)
    assert call(big) == _abi.MT_ERR_UNSUPPORTED and "960x540" in err()
    with pytest.raises(m.MtgpuError) as ei:
        big.activity_map(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)), [0, 1])
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)

    for rb in (0, 7, 16, 39, 41, -8):
        assert call(s, rb=rb) == inv and "rec_bytes" in err()
    assert call(s, rec_ptr=rec.data_ptr() + 4) == inv and "d_rec" in err() and "8-byte" in err()
    assert call(s, o=0) == inv and "d_frame_off" in err()
    assert call(s, so=0) == inv and "d_stream_off" in err()
    assert call(s, o=off.data_ptr() + 4) == inv and "d_frame_off" in err()
    assert call(s, a=None, c=None, f=None) == inv and "all NULL" in err()
    assert call(s, a=outs["active"].data_ptr() + 2) == inv and "d_active" in err()
    # outputs must be memory of the context's device: the flush uses global atomics
    assert call(s, a=pinned.data_ptr()) == inv and "d_active" in err() and "atomics" in err()
    assert call(s, a=None, c=pinned.data_ptr()) == inv and "d_centre" in err()
    assert call(s, a=None, c=None, f=pinned.data_ptr()) == inv and "d_frames" in err()
    # the host entry point validates its offsets
    one = np.zeros(1, dtype=np.uint32)
    o_h, p1 = np.array([0, 4, 8], dtype=np.uint64), one.ctypes.data_as(C.c_void_p)
    mvh = np.zeros(8, dtype=m.MV_DTYPE)

    def host(off_h, soff_h, n_streams):
        return lib.mtgpu_activity_map(s._ctx, mvh.ctypes.data_as(C.c_void_p), off_h.ctypes.data_as(C.c_void_p), None, 2,
                                      soff_h.ctypes.data_as(C.c_void_p), n_streams, 0, None, None, p1)

    assert host(o_h, np.array([0, 2, 1], dtype=np.uint64), 2) == inv and "stream_off" in err()
    assert host(o_h, np.array([0, 1], dtype=np.uint64), 1) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(np.array([0, 9, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64), 1) == inv and "frame_off" in err()
    assert lib.mtgpu_activity_map(s._ctx, None, None, None, 0, np.zeros(1, dtype=np.uint64).ctypes.data_as(C.c_void_p), 0, 0,
                                  None, None, None) == inv and "all NULL" in err()
    torch.cuda.synchronize()
    for t in list(outs.values()) + [pinned]:
        assert int((t != JUNK).sum()) == 0           # nothing was launched: no output word changed
    assert one[0] == 0
    assert call(s) == _abi.MT_OK                       # and the same call with valid arguments runs
    torch.cuda.synchronize()
    for t in outs.values():
        assert int((t == JUNK).sum()) == 0


# ------------------------------------------------------------------ 9. exact extent

def test_exactly_the_block_is_written(gpu_scanner_factory):
    """Outputs as views into larger junk tensors: the stated sizes hold the maps, the words before and behind are
    unchanged.  With one plane NULL the other outputs are right and its would-be memory is untouched.  n_frames == 0
    clears."""
    import torch
    mv, off, sd = parity_input()
    p, want = parity_model(0, 0)
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_soff = soff_tensor(STREAMS_1)
    plane = 3 * 68 * 120
    PAD = 64

    def run(want_names, n_frames=128):
        bufs = {n: torch.full(((3 if n == "frames" else plane) + 2 * PAD,), JUNK, dtype=torch.int32, device="cuda")
                for n in ("active", "centre", "frames")}
        torch.cuda.synchronize()
        ptr = {n: (bufs[n][PAD:].data_ptr() if n in want_names else None) for n in bufs}
        _abi.check(s._lib.mtgpu_activity_map_device(s._ctx, d_rec.data_ptr(), 8, len(mv), d_off.data_ptr(), d_sd.data_ptr(), n_frames,
                                                    d_soff.data_ptr(), 3, 0, 0, ptr["active"], ptr["centre"], ptr["frames"],
                                                    torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return {n: b.cpu().numpy() for n, b in bufs.items()}

    for names in (("active", "centre", "frames"), ("centre", "frames"), ("active", "frames"), ("active", "centre"), ("frames",)):
        raw = run(names)
        for i, n in enumerate(("active", "centre", "frames")):
            size = 3 if n == "frames" else plane
            assert (raw[n][:PAD] == JUNK).all() and (raw[n][PAD + size:] == JUNK).all(), (names, n)
            if n in names:
                assert np.array_equal(raw[n][PAD:PAD + size].view(np.uint32), want[i].reshape(-1)), (names, n)
            else:
                assert (raw[n] == JUNK).all(), (names, n)
    raw = run(("active", "centre", "frames"), n_frames=0)
    for n in raw:
        size = 3 if n == "frames" else plane
        assert (raw[n][PAD:PAD + size] == 0).all() and (raw[n][:PAD] == JUNK).all() and (raw[n][PAD + size:] == JUNK).all()
    a, c, f = s.activity_map(m.FrameBatch(mv[:0], off[:1], None, None), [0, 0, 0])
    assert a.shape == (2, 68, 120) and not a.any() and not c.any() and f.tolist() == [0, 0]


# ------------------------------------------------------------------ 10. two threads, one context

def test_two_threads_on_their_own_streams(gpu_scanner_factory):
    import torch
    mv, off, sd = parity_input()
    p, want = parity_model(0, 0)
    s = gpu_scanner_factory(p)
    d40 = to_device(mv, off, sd, False)
    d8 = to_device(mv, off, sd, True)
    d_soff = soff_tensor(STREAMS_1)
    torch.cuda.synchronize()
    results, errors = [[], []], []

    def work(i):
        try:
            st = torch.cuda.Stream()
            d_rec, d_off, d_sd = d8 if i else d40
            outs = [junk_maps(s, 3) for _ in range(4)]
            torch.cuda.synchronize()                  # the junk fill ran on torch's stream, the calls run on `st`
            for j, out in enumerate(outs):
                s.activity_map_device(d_rec, d_off, d_sd, d_soff, run_frames=(0, 1, 3, 64)[j], compact=bool(i), out=out,
                                      stream=st.cuda_stream)
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
            got = tuple(out[n].cpu().numpy().view(np.uint32) for n in ("active", "centre", "frames"))
            assert_maps_equal(got, want[:3], f"thread {i}")


# ------------------------------------------------------------------ 11. profiling

def test_profiled_call_records_one_triple(gpu_scanner_factory):
    mv, off, sd = parity_input()
    p, want = parity_model(0, 0)
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(STREAMS_1), False)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert_maps_equal(got, want[:3], "profiled")


# ------------------------------------------------------------------ 12. end to end

def test_end_to_end_command(tmp_path):
    """A .mtmv written with mvfile, then `python -m mvtrim_amd.activity --json --vertical-mask 0,0.05,0.1 --npy` in a
    fresh child process: the row table, the margins (0, 3 and 6 rows of 68) and the .npy contents equal the model's on
    the unmasked grid."""
    F = 48
    spec = synth.spec_1080p(seed=41, sub=1, event_records=3)
    spec.events = synth.scripted_events(spec, F)
    frames = [synth.gen_frame(spec, f) for f in range(F)]
    path = str(tmp_path / "stream.mtmv")
    m.mvfile.write_mtmv(path, spec.width, spec.height, 1, spec.tb_den, spec.fps, F / spec.fps,
                        [spec.pts_ticks(f) for f in range(F)], frames)
    b = m.FrameBatch.from_frames(frames)
    p = m.ScanParams.from_config(1920, 1080, vertical_mask=0.0)
    for kept in (False, True):
        mc = max(1, p.clusters_needed) if kept else 0
        active, centre, nfr, _ = model_maps(p, b.mv, b.frame_off, b.has_sd, [0, F], mc)
        assert_oracle_identities(p, b.mv, b.frame_off, b.has_sd, [0, F], mc, centre, nfr, "model")
        tot = int(centre.sum())
        assert tot > 0 and 0 < int(nfr[0]) <= F
        prefix = str(tmp_path / ("kept" if kept else "all"))
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-m", "mvtrim_amd.activity", path, "--json", "--vertical-mask", "0,0.05,0.1",
                              "--npy", prefix] + (["--kept"] if kept else []), capture_output=True, text=True, env=env, cwd=ROOT,
                             timeout=300)
        assert out.returncode == 0, out.stderr
        doc = json.loads(out.stdout)
        assert (doc["grid_w"], doc["grid_h"], doc["frames"], doc["contributing_frames"], doc["min_centres"]) == (120, 68, F, int(nfr[0]), mc)
        assert [(r["row"], r["active"], r["centre"]) for r in doc["rows"]] == \
            [(y, int(active[0, y].sum()), int(centre[0, y].sum())) for y in range(68)]
        assert [r["centre_share"] for r in doc["rows"]] == [int(centre[0, y].sum()) / tot for y in range(68)]
        assert [r["margin_rows"] for r in doc["vertical_mask"]] == [0, 3, 6]
        assert [r["centre_share_dropped"] for r in doc["vertical_mask"]] == \
            [(tot - int(centre[0, k:68 - k].sum())) / tot for k in (0, 3, 6)]
        assert all("estimate" in r["kind"] and "not the count a masked scan returns" in r["kind"] for r in doc["vertical_mask"])
        assert np.array_equal(np.load(prefix + "_active.npy"), active[0]) and np.array_equal(np.load(prefix + "_centre.npy"), centre[0])


def test_plain_c_activity_example(tmp_path):
    """examples/activity_example.c: the maps of two tiny streams from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "activity_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "activity_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all frames:  stream 0: 30 frames, clock cell (101, 0) centre in 30, object cell (41, 30) centre in 10" in out.stdout
    assert "69 % of the centre counts lie in row 0" in out.stdout and "kept frames: stream 0: 30, stream 1: 30" in out.stdout
