"""Inputs of tests/test_gpu_pipe_zones.py (a keep mask carried through the pipe, include/mtgpu_pipe_zones.h), built once
and frozen.  The expected value of every case is the oracle on the same frames with every record removed whose destination
cell is ignored, has_sd unchanged (zones_inputs.oracle_batch: the equivalence include/mtgpu_zones.h states for
vectors_needed >= 1) — or a count derived by hand where the case says so.  tests/test_pipe_zones_host.py checks, without
a GPU, that the masks below do to these frames what the GPU cases need them to do."""
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import synth, zones

import zones_inputs as zi
from derived_edge_inputs import frozen, voters


def batch_arrays(frames):
    """frames (MV_DTYPE arrays / None) -> (mv, off, sd) as one stream."""
    b = m.FrameBatch.from_frames(frames)
    return (np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
            np.ascontiguousarray(b.has_sd, dtype=np.uint8))


def expect(p, frames, keep):
    """(flags uint8 [F], centres uint32 [F]) under `keep` (bool [gh, gw]; None: no mask): the oracle on the filtered
    records."""
    mv, off, sd = batch_arrays(frames)
    k = np.ones((1, p.grid_h, p.grid_w), dtype=bool) if keep is None else np.asarray(keep, dtype=bool)[None]
    fl, ce, _ = zi.oracle_batch(p, mv, off, sd, np.array([0, len(frames)], dtype=np.uint64), k)
    return fl, ce


# ------------------------------------------------------------------ 1. the 90-frame 1080p recording

HD_KW = dict(vectors_needed=1)
# Three objects (synth.Event: frames [f0, f1), first cell, size in cells, motion): A crosses the zone that MASK_A
# ignores entirely, B is cut in half by it, C never touches it.
EVENTS = [synth.Event(3, 46, 10, 20, 4, 3, 8, 2), synth.Event(48, 71, 80, 40, 6, 4, -6, 3), synth.Event(72, 89, 50, 10, 5, 3, 7, -2)]
# cells [x0, x1) x [y0, y1): A's whole path (it drifts 5 cells to the right), the two upper rows of B
MASK_A_RECTS = [(8, 18, 24, 26), (74, 40, 90, 42)]
# another recording's zones: C's whole path and nothing else
MASK_B_RECTS = [(48, 8, 62, 15)]
EMPTY_FRAME, DENSE_FRAME = 7, 40


@functools.lru_cache(maxsize=None)
def hd_case():
    """(params, frames[90], pts[90], keep A, keep B, {name: (flags, centres)} for "none", "a", "b").  Frames 0, 30 and
    60 have no side data (None), frame 7 has side data and no record, frame 40 comes from a denser stream."""
    p = m.ScanParams.from_config(1920, 1080, **HD_KW)
    spec = synth.spec_1080p(seed=17, sub=1)
    spec.events = list(EVENTS)
    frames = [synth.gen_frame(spec, i) for i in range(90)]
    frames[EMPTY_FRAME] = np.zeros(0, dtype=m.MV_DTYPE)
    dense = synth.spec_1080p(seed=18, sub=2)
    dense.events = list(EVENTS)
    frames[DENSE_FRAME] = synth.gen_frame(dense, DENSE_FRAME)
    for f in frames:
        if f is not None:
            f.setflags(write=False)
    keep_a = zones.keep_from_rects(p, MASK_A_RECTS, unit="cell")
    keep_b = zones.keep_from_rects(p, MASK_B_RECTS, unit="cell")
    want = {"none": frozen(*expect(p, frames, None)), "a": frozen(*expect(p, frames, keep_a)), "b": frozen(*expect(p, frames, keep_b))}
    pts = [spec.pts_seconds(i) for i in range(90)]
    frozen(keep_a, keep_b)
    return p, tuple(frames), tuple(pts), keep_a, keep_b, want


# ------------------------------------------------------------------ 4. stale results in a pinned block

@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, batch 1 frames, batch 2 frames, keep): every frame of batch 1 moves outside the zone (flag 1, count 2);
    batch 2 — the same number of frames, into the same block — alternates frames without side data and frames whose
    whole motion lies inside the zone."""
    p = m.ScanParams.from_config(1920, 1080, **HD_KW)
    keep = zones.keep_from_rects(p, [(30, 30, 40, 40)], unit="cell")
    one = [voters([(60 + i, 20, 1, 5, 0), (61 + i, 20, 1, 5, 0)]) for i in range(12)]
    two = [None if i % 2 == 0 else voters([(32, 33, 1, 5, 0), (33, 33, 1, 5, 0), (33, 34, 1, 5, 0)]) for i in range(12)]
    frozen(keep)
    return p, tuple(one), tuple(two), keep


# ------------------------------------------------------------------ 5. the word seam, by hand

@functools.lru_cache(maxsize=None)
def seam_case():
    """(params, frames, [(keep, hand centres per frame)]) on the 120-wide grid (W = 2): frame 0 holds one pair of
    active cells at columns 63 and 64 of row 30 — the last bit of word 0 and the first of word 1.  Each is the other's
    only neighbour: 2 centres; with either bit cleared the other cell has no neighbour left: 0.  A carry taken from the
    unmasked neighbour word would count 1."""
    p = m.ScanParams.from_config(1920, 1080, **HD_KW)
    assert (p.grid_w + 63) // 64 == 2
    frames = (voters([(63, 30, 1, 5, 0), (64, 30, 1, 5, 0)]),)
    cases = []
    for cleared, hand in ((None, 2), ((63, 30), 0), ((64, 30), 0)):
        keep = np.ones((p.grid_h, p.grid_w), dtype=bool)
        if cleared:
            keep[cleared[1], cleared[0]] = False
        cases.append((keep, (hand,)))
    return p, frames, cases


@functools.lru_cache(maxsize=None)
def vn0_case():
    """(params, frames, keep, hand): vectors_needed == 0 on a 10 x 8 grid without a margin, ONE frame with side data and
    no record: every kept cell is active, every ignored one is not (this is not record removal).  keep = the 2 x 2 block
    (3..4, 3..4) and the single cell (7, 6): each cell of the block has two kept neighbours — 4 centres; (7, 6) has none."""
    p = m.ScanParams.from_config(160, 128, vertical_mask=0.0, vectors_needed=0, clusters_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (10, 8, 0)
    keep = np.zeros((8, 10), dtype=bool)
    keep[3:5, 3:5] = True
    keep[6, 7] = True
    return p, (np.zeros(0, dtype=m.MV_DTYPE),), keep, (4,)


# ------------------------------------------------------------------ 6. other grids

@functools.lru_cache(maxsize=None)
def uhd_case():
    """(params, frames[12], keep, (flags, centres)): 4K, 240 x 135 cells, W = 4; one object that the zone cuts."""
    p = m.ScanParams.from_config(3840, 2160, **HD_KW)
    assert (p.grid_w, p.grid_h) == (240, 135)
    spec = synth.spec_4k(seed=5, sub=1, gop=5)
    spec.events = [synth.Event(1, 12, 120, 60, 12, 5, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(12)]
    keep = zones.keep_from_rects(p, [(126, 58, 200, 63)], unit="cell")      # columns 126.. of the object's upper rows
    return p, tuple(frames), keep, frozen(*expect(p, frames, keep))


TALL_W, TALL_H = 64, 16800


@functools.lru_cache(maxsize=None)
def tall_case():
    """(params, frames, keep, hand centres): a 4 x 1050 grid without a margin — 1050 keep words of the analysed rows, more
    than the 1024 lanes of a workgroup stage in one trip.  Frame 0: vertical pairs of active cells in column 1 at rows
    (5, 6), (1030, 1031) and (1040, 1041); the zone ignores (1, 1031) and nothing else.  Unmasked 6; masked: rows 5, 6
    and 1040, 1041 count, 1030 has lost its only neighbour: 4.  Frame 1: the pair (1, 1030), (2, 1030) only: 2 under
    either mask.  Keep words 1024.. come from the second staging trip."""
    p = m.ScanParams.from_config(TALL_W, TALL_H, vertical_mask=0.0, vectors_needed=1, clusters_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (4, 1050, 0)
    f0 = voters([(1, y, 1, 5, 0) for y in (5, 6, 1030, 1031, 1040, 1041)])
    f1 = voters([(1, 1030, 1, 5, 0), (2, 1030, 1, 5, 0)])
    keep = np.ones((1050, 4), dtype=bool)
    keep[1031, 1] = False
    return p, (f0, f1), keep, (4, 2)


FINE_KW = dict(block_size=4, block_shift=2, vectors_needed=1)      # 960 x 540 cells: no masked form
