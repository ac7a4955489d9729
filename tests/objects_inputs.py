"""Inputs of tests/test_gpu_objects.py and tests/test_objects_host.py (the object scan, include/mtgpu_objects.h), with the
expected lists written out BY HAND where a case says so and from tests/objects_model.py elsewhere.  Built once per
process and handed out read-only.  An entry is (cells, first, x0, y0, x1, y1); first = y * gw + x of the blob's first cell
in row-major order."""
import collections
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import objects

import blob_planes as bp
import blobs_inputs as bi
import derived_cliff_inputs as dci
import objects_model as om
from derived_edge_inputs import MI355X_LDS, frozen

TABLE_BYTES = 24                                  # MT_OBJECT_TABLE_BYTES: a 64-bit key and four 32-bit bounds per entry
Case = collections.namedtuple("Case", "p mv off sd soff keeps hand")


def cells_plane(gw, gh, cells):
    a = np.zeros((gh, gw), dtype=bool)
    for x, y in cells:
        a[y, x] = True
    return a


def run(x, y, n):
    return [(x + i, y) for i in range(n)]


# ------------------------------------------------------------------ 1. three blobs on the smallest grid

HAND_GRID = bp.GRIDS["63x12"]
HAND_A = [(10, 2), (11, 2), (10, 3)]              # first (10, 2): 2 * 63 + 10 = 136
HAND_B = [(3, 6), (4, 6), (5, 6)]                 # first (3, 6): 6 * 63 + 3 = 381 — further left, later in row-major order
HAND_C = [(20, 9), (21, 9)]                       # first (20, 9): 9 * 63 + 20 = 587
HAND_LIST = [(3, 136, 10, 2, 11, 3), (3, 381, 3, 6, 5, 6), (2, 587, 20, 9, 21, 9)]


@functools.lru_cache(maxsize=None)
def hand_case():
    """63 x 12, margin 0, four frames: 0 the blobs A, B, C (3, 3 and 2 cells; every cell has a neighbour in its blob, so
    all 8 are centres; A and B tie and A holds the smaller first); 1 without side data; 2 with side data and no record;
    3 frame 0 again.  soff (0, 3) with one all-ones plane: under the mask frame 3 lies behind the last stream.
    hand: {"plain": ..., "masked": ...} -> per frame (centres, blobs, [entries])."""
    g = HAND_GRID
    p = bp.params_of(g)
    three = bi.cells_frame(HAND_A + HAND_B + HAND_C)
    mv, off, sd = bi.batch_of([three, None, np.zeros(0, dtype=m.MV_DTYPE), three], 41)
    assert sd.tolist() == [1, 0, 1, 1]
    full, none = (8, 3, HAND_LIST), (0, 0, [])
    keeps = np.ones((1, g.gh, g.gw), dtype=bool)
    return Case(p, *frozen(mv, off, sd, np.array([0, 3], dtype=np.uint64), keeps),
                {"plain": [full, none, none, full], "masked": [full, none, none, none]})


def hand_want(rows, k, min_blob_cells=1):
    """[(centres, blobs, [entries])] per frame -> the dict objects_model.model_batch returns, at k entries per frame."""
    F = len(rows)
    out = {"centres": np.array([r[0] for r in rows], dtype=np.uint32), "blobs": np.array([r[1] for r in rows], dtype=np.uint32),
           "objects": np.array([sum(1 for e in r[2] if e[0] >= max(1, min_blob_cells)) for r in rows], dtype=np.uint32),
           "list": np.zeros((F, k), dtype=om.OBJECT_DTYPE)}
    for f, r in enumerate(rows):
        out["list"][f] = om.entries(r[2], k)
    return out


# ------------------------------------------------------------------ 3. more candidates in one word than k

PAIRS_ROW, PAIRS = 10, 21


@functools.lru_cache(maxsize=None)
def pairs_case():
    """120 x 68, margin 3, one frame: on row 10 the pairs (1, 2), (4, 5) .. (61, 62) — 21 blobs of 2 cells, all in word 0 of
    that row.  hand: the 21 entries in list order (equal sizes: by first, i.e. from left to right)."""
    p = bi.grid(120, 68, margin=3)
    cells = [c for i in range(PAIRS) for c in run(1 + 3 * i, PAIRS_ROW, 2)]
    assert cells[-1] == (62, PAIRS_ROW)
    mv, off, sd = bi.batch_of([bi.cells_frame(cells)], 42)
    hand = [(2, PAIRS_ROW * 120 + 1 + 3 * i, 1 + 3 * i, PAIRS_ROW, 2 + 3 * i, PAIRS_ROW) for i in range(PAIRS)]
    return Case(p, *frozen(mv, off, sd), None, None, [(2 * PAIRS, PAIRS, hand)])


# ------------------------------------------------------------------ 4. word seams for ranks above 0

SEAM_GRID = bp.GRIDS["wide-2000x9"]
SEAM_BARS = [(60, 1, 11), (120, 3, 16), (1000, 5, 31)]      # (x, y, cells): across columns 64, 128 and 1024
SEAM_BIG = [(300, 7, 19), (300, 8, 19)]                     # two rows inside word 4 (columns 256 .. 319): 38 cells
SEAM_LIST = [(38, 7 * 2000 + 300, 300, 7, 318, 8), (31, 5 * 2000 + 1000, 1000, 5, 1030, 5), (16, 3 * 2000 + 120, 120, 3, 135, 3),
             (11, 1 * 2000 + 60, 60, 1, 70, 1)]


@functools.lru_cache(maxsize=None)
def seams_case():
    """2000 x 9, margin 0, one frame: three bars of 11, 16 and 31 cells, each across a 64-column seam, and a blob of 38
    cells elsewhere, so that the three are ranks 3, 2 and 1.  hand: the four entries."""
    g = SEAM_GRID
    p = bp.params_of(g)
    a = cells_plane(g.gw, g.gh, [c for x, y, n in SEAM_BARS + SEAM_BIG for c in run(x, y, n)])
    for x, y, n in SEAM_BARS:
        assert x // 64 != (x + n - 1) // 64
    mv, off, sd = bi.batch_of([bp.plane_frame(a, p.block_shift)], 43)
    return Case(p, *frozen(mv, off, sd), None, None, [(int(a.sum()), 4, SEAM_LIST)])


# ------------------------------------------------------------------ 5. three streams for the sweep

STREAM_FRAMES, STREAMS, FPS = 24, 3, 25.0
SWEEP_LEVELS = (1, 2, 4)
SWEEP_MIN_BLOB = 2


@functools.lru_cache(maxsize=None)
def streams_case():
    """(params 120 x 68 margin 3 CLUSTERS_NEEDED 1, mv, off, sd, pts, soff): three streams of 24 frames at 25 fps.  Frame
    f of stream s holds n = ((f + 4 * s) // 3) % 6 blobs: blob i is a run of 2 + i % 3 cells on row 5 + 3 * i from column
    10, and a single cell — no centre — at (40, 5 + 3 * i)."""
    p = bi.grid(120, 68, margin=3)
    frames = []
    for s in range(STREAMS):
        for f in range(STREAM_FRAMES):
            n = ((f + 4 * s) // 3) % 6
            frames.append(bi.cells_frame([c for i in range(n) for c in run(10, 5 + 3 * i, 2 + i % 3) + [(40, 5 + 3 * i)]]))
    mv, off, sd = bi.batch_of(frames, 44)
    pts = np.tile(np.arange(STREAM_FRAMES, dtype=np.float64) / FPS, STREAMS)
    soff = np.arange(STREAMS + 1, dtype=np.uint64) * STREAM_FRAMES
    return (p,) + frozen(mv, off, sd, pts, soff)


def stream_objects():
    """objects[f] of streams_case by construction, at min_blob_cells 1 .. 2 (every blob has at least two cells)."""
    return np.array([((f + 4 * s) // 3) % 6 for s in range(STREAMS) for f in range(STREAM_FRAMES)], dtype=np.uint32)


# ------------------------------------------------------------------ 6. the cliff

CLIFF_GW = 65


def lds_by_hand(gw, R, k):
    """csrc/objects_kernels.h: the blob scan's layout and, behind it, k entries of the ranking table."""
    return bi.lds_by_hand(gw, R) + k * TABLE_BYTES


def objects_preview_or_none(p, k, lds=MI355X_LDS):
    try:
        return objects.preview(p, k, lds)
    except m.MtgpuError as e:
        if e.code != m._abi.MT_ERR_UNSUPPORTED:
            raise
        return None


@functools.lru_cache(maxsize=None)
def cliff_rows(k):
    """The tallest 65-column grid mtgpu_objects_preview accepts for k entries at 163 840 bytes, by bisection."""
    return bi._largest(lambda gh: objects_preview_or_none(bi.limit_params(CLIFF_GW, gh), k) is not None, 16383)


@functools.lru_cache(maxsize=None)
def cliff_case(k):
    """65 x cliff_rows(k), margin 0, two frames: a serpentine over the whole grid (one blob), and twenty runs of 2 .. 21
    cells on every second row upwards from the LAST row — the labels and the centre words at the end of the layout."""
    gh = cliff_rows(k)
    p = bi.limit_params(CLIFF_GW, gh, vectors_needed=1, clusters_needed=1)
    snake = cells_plane(CLIFF_GW, gh, bi.serpentine_cells(CLIFF_GW, 0, gh)[0])
    runs = cells_plane(CLIFF_GW, gh, [c for i in range(20) for c in run(1 + i, gh - 1 - 2 * i, 2 + i)])
    mv, off, sd = bi.batch_of([bp.plane_frame(snake, p.block_shift), bp.plane_frame(runs, p.block_shift)], 45)
    return Case(p, *frozen(mv, off, sd), None, None, None)


# ------------------------------------------------------------------ 2. the centre planes of blob_planes

@functools.lru_cache(maxsize=None)
def expected(name):
    """objects_model.model_batch of blob_planes.batch(name) at k = 16 and min_blob_cells 1, read-only."""
    b = bp.batch(name)
    out = om.model_batch(b.p, b.mv, b.off, b.sd, om.K_MAX, 1, b.soff, b.keeps)
    frozen(*out.values())
    return out
