"""Inputs of tests/test_gpu_pipe_blobs.py (motion blobs carried through the pipe, include/mtgpu_pipe_blobs.h), built
once and frozen.  Every expected value is either derived by hand in the docstring of its case or comes from
tests/blobs_model.py (the flood-fill model); tests/test_pipe_blobs_host.py checks, without a GPU, that the model returns
every hand-derived number below."""
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import synth

import blobs_inputs as bi
import blobs_model as bm
from blobs_inputs import cells_frame, grid
from derived_edge_inputs import frozen

GW, GH = 120, 68            # the 1080p grid's shape (two keep words per row: a word seam at x = 63 / 64), margin 0 here

PAIRS = [(10, 10), (11, 10), (30, 20), (31, 20), (70, 40), (71, 40), (100, 60), (101, 60)]      # four pairs in interior columns
BLOCK = [(x, y) for y in (30, 31) for x in range(40, 44)]                                        # 2 rows x 4 columns
BIG = [(x, y) for y in (12, 13, 14) for x in range(20, 24)]                                      # 3 rows x 4 columns
LONE = [(50, 50)]                                                                                # votes, no neighbour: no centre


def block(x0, y0, w, h):
    return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]


def batch_arrays(frames):
    """frames (MV_DTYPE arrays / None) -> (mv, off, sd) as one stream."""
    b = m.FrameBatch.from_frames(list(frames))
    return (np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
            np.ascontiguousarray(b.has_sd, dtype=np.uint8))


def model(p, frames, keep=None):
    """{"centres", "largest", "blobs": [F]} lists of the flood-fill model on the frames as one stream under `keep`
    (bool [gh, gw]; None: no mask)."""
    mv, off, sd = batch_arrays(frames)
    if keep is None:
        out = bm.model_batch(p, mv, off, sd)
    else:
        out = bm.model_batch(p, mv, off, sd, np.array([0, len(frames)], dtype=np.uint64), np.asarray(keep, dtype=bool)[None])
    return {k: out[k].tolist() for k in ("centres", "largest", "blobs")}


def flags_of(p, mo, min_blob_cells):
    return bm.flags_np(p, mo["centres"], mo["largest"], min_blob_cells).tolist()


def freeze(frames):
    for f in frames:
        if f is not None:
            f.setflags(write=False)
    return tuple(frames)


# ------------------------------------------------------------------ 1. the rule bites

@functools.lru_cache(maxsize=None)
def bite_case():
    """(params, frames, hand).  120 x 68, margin 0, CLUSTERS_NEEDED 8, VECTORS_NEEDED 1.
    Frame A: four pairs, far apart.  Each cell's only active neighbour is its partner: 8 centres, 4 blobs of 2.
    Frame B: a block of 2 rows x 4 columns: every cell has a neighbour in the block: 8 centres, 1 blob of 8."""
    p = grid(GW, GH, 0, vn=1, cn=8)
    hand = {"centres": [8, 8], "blobs": [4, 1], "largest": [2, 8]}
    return p, freeze([cells_frame(PAIRS), cells_frame(BLOCK)]), hand


# ------------------------------------------------------------------ 2. every layout and batch shape

@functools.lru_cache(maxsize=None)
def shapes_case():
    """(params, frames[14]): frames without side data first, in the middle and last; a frame with side data and no
    record; ragged frames (1 .. 48 records, several votes per cell in one of them); every kind of answer (no centre;
    centres pass and the blob rule fails; both pass; centres fail)."""
    p = grid(GW, GH, 0, vn=1, cn=8)
    seam = [(x, 25) for x in range(58, 70)]                          # one run of 12 across x = 63 / 64
    heavy = bi.voters([(x, y, 3, 5, 0) for x, y in BLOCK])           # three votes per cell: 24 records, the block's answer
    frames = [None, cells_frame(PAIRS), cells_frame(BLOCK), cells_frame(BIG + PAIRS), np.zeros(0, dtype=m.MV_DTYPE),
              cells_frame(LONE), None, cells_frame(seam), heavy, cells_frame(block(0, 0, 6, 8)), cells_frame(PAIRS[:4]),
              cells_frame(BLOCK + PAIRS + seam), cells_frame(block(114, 60, 6, 8)), None]
    return p, freeze(frames)


MIN_BLOB = 3


# ------------------------------------------------------------------ 3. the seam, the largest union

@functools.lru_cache(maxsize=None)
def seam_case():
    """(params, frames, hand) on 120 x 68, margin 0, CLUSTERS_NEEDED 1.
    Frame 0: one run on row 10, columns 60 .. 67: it crosses x = 63 / 64.  8 centres, 1 blob of 8.
    Frame 1: columns 58 .. 63 on row 20 and 63 .. 70 on row 21: the runs touch only at column 63, the last bit of word
             0; the lower run crosses the seam.  6 + 8 = 14 centres, 1 blob.
    Frame 2: columns 64 .. 70 on row 30 and 60 .. 64 on row 31: they touch only at column 64, the first bit of word 1.
             7 + 5 = 12 centres, 1 blob.
    Frame 3: columns 60 .. 63 on row 40 and 64 .. 67 on row 41: the runs end and begin at the seam and do NOT touch
             (a diagonal is no contact).  8 centres, 2 blobs of 4."""
    p = grid(GW, GH, 0, vn=1, cn=1)
    frames = [cells_frame([(x, 10) for x in range(60, 68)]),
              cells_frame([(x, 20) for x in range(58, 64)] + [(x, 21) for x in range(63, 71)]),
              cells_frame([(x, 30) for x in range(64, 71)] + [(x, 31) for x in range(60, 65)]),
              cells_frame([(x, 40) for x in range(60, 64)] + [(x, 41) for x in range(64, 68)])]
    hand = {"centres": [8, 14, 12, 8], "blobs": [1, 1, 1, 2], "largest": [8, 14, 12, 4]}
    return p, freeze(frames), hand


@functools.lru_cache(maxsize=None)
def vn0_case():
    """(params, frames, hand): VECTORS_NEEDED 0 at margin 0, one frame with side data and no record: every cell is
    active, every cell of columns 1 .. 118 is a centre, all of them one blob: largest == centres == 118 x 68 = 8024."""
    p = grid(GW, GH, 0, vn=0, cn=1)
    return p, freeze([np.zeros(0, dtype=m.MV_DTYPE)]), {"centres": [118 * 68], "blobs": [1], "largest": [118 * 68]}


# ------------------------------------------------------------------ 4. mask and blobs together

MASK_MIN_BLOB = 5


@functools.lru_cache(maxsize=None)
def mask_case():
    """(params, frames, keep, hand unmasked, hand masked).  120 x 68, margin 0, CLUSTERS_NEEDED 8.  The keep mask clears
    columns 42 and 82 on every row.
    Frame 0: the block of 2 x 4 at columns 40 .. 43.  Unmasked 8 centres, 1 blob of 8.  Masked: columns 40 .. 41 remain
             as 2 x 2 = 4 cells and column 43 as 2 x 1 = 2 cells: 6 centres, 2 blobs, largest 4.
    Frame 1: a block of 2 x 5 at columns 80 .. 84.  Unmasked 10 centres, 1 blob of 10.  Masked: 2 x 2 = 4 per half:
             8 centres, 2 blobs, largest 4 — the centre rule still passes, only the blob rule (>= 5) fails."""
    p = grid(GW, GH, 0, vn=1, cn=8)
    keep = np.ones((GH, GW), dtype=bool)
    keep[:, 42] = False
    keep[:, 82] = False
    frozen(keep)
    frames = [cells_frame(BLOCK), cells_frame(block(80, 30, 5, 2))]
    plain = {"centres": [8, 10], "blobs": [1, 1], "largest": [8, 10]}
    masked = {"centres": [6, 8], "blobs": [2, 2], "largest": [4, 4]}
    return p, freeze(frames), keep, plain, masked


# ------------------------------------------------------------------ 5. stale results in a reused pinned block

@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, batch 1, batch 2, hand 1, hand 2).  CLUSTERS_NEEDED 8, min_blob_cells 3.
    Batch 1: three frames, each the block of 3 x 4: 12 centres, largest 12, flag 1.
    Batch 2, into the same slots: the four pairs (8 centres pass, largest 2 fails: flag 0 — the store at the end of the
    labelling passes); one lone cell (votes, no centre: 0 / 0 / flag 0 — the store of the early exit); no side data
    (0 / 0 / flag 0 — the planning kernel's store)."""
    p = grid(GW, GH, 0, vn=1, cn=8)
    one = [cells_frame(BIG) for _ in range(3)]
    two = [cells_frame(PAIRS), cells_frame(LONE), None]
    h1 = {"flags": [1, 1, 1], "centres": [12, 12, 12], "largest": [12, 12, 12]}
    h2 = {"flags": [0, 0, 0], "centres": [8, 0, 0], "largest": [2, 0, 0]}
    return p, freeze(one), freeze(two), h1, h2


# ------------------------------------------------------------------ 7. the 4K grid

@functools.lru_cache(maxsize=None)
def uhd_case():
    """(params, frames[6]): 240 x 135 cells (W = 4), the 4K margin of 6 rows, CLUSTERS_NEEDED 4: a large blob, several
    small ones at the three word seams and on the first and last analysed rows, both in one frame, a frame with side data
    and no record, a frame without side data.  Expected values: the model."""
    p = m.ScanParams.from_config(3840, 2160, vectors_needed=1, clusters_needed=4)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (240, 135, 6)
    large = block(100, 50, 40, 9)
    small = [(63, 20), (64, 20), (127, 30), (128, 30), (191, 40), (192, 40), (10, 6), (11, 6), (200, 128), (201, 128),
             (5, 2), (6, 2)]                                                 # the last pair lies in the margin: no centre
    frames = [cells_frame(large), cells_frame(small), cells_frame(large + small), np.zeros(0, dtype=m.MV_DTYPE), None,
              cells_frame(block(1, 6, 238, 2))]
    return p, freeze(frames)


FINE_KW = dict(block_size=4, block_shift=2, vectors_needed=1)      # 960 x 540 cells: no blob form


# ------------------------------------------------------------------ 9 / 11. the recording

REC_FRAMES, REC_FPS = 48, 25.0


@functools.lru_cache(maxsize=None)
def recording_case():
    """(params, frames[48], pts[48], keep): stream 0 of blobs_inputs.sweep_case at the default CLUSTERS_NEEDED 2 — frame
    f holds a run of (1, 2, 4, 9)[(f // 6) % 4] cells from column 40 of row 30 and four separate pairs.  largest is 2, 2,
    4, 9: min_blob_cells 4 keeps half of the frames, 8 a quarter.  keep clears column 44 on every row: the run of 9
    becomes 4 + 4, and min_blob_cells 8 keeps nothing."""
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1)
    assert (p.grid_w, p.grid_h, p.clusters_needed) == (GW, GH, 2)
    _, mv, off, _, _, _ = bi.sweep_case()
    frames = [np.array(mv[int(off[f]):int(off[f + 1])]) for f in range(REC_FRAMES)]
    keep = np.ones((GH, GW), dtype=bool)
    keep[:, 44] = False
    frozen(keep)
    # pts as the host layer computes them from a .mtmv with time base 1 / 25: frame->pts * av_q2d(time_base) (:361)
    return p, freeze(frames), tuple(float(f) * (1.0 / REC_FPS) for f in range(REC_FRAMES)), keep


REC_LARGEST = [(2, 2, 4, 9)[(f // 6) % 4] for f in range(REC_FRAMES)]
REC_LARGEST_MASKED = [(2, 2, 4, 4)[(f // 6) % 4] for f in range(REC_FRAMES)]
