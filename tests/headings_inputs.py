"""Inputs of tests/test_gpu_headings.py and tests/test_headings_host.py (the heading scan, include/mtgpu_headings.h), with
the expected numbers written out BY HAND where a case says so and from tests/headings_model.py elsewhere.  Built once
per process and handed out read-only.  A motion entry is (n[8], records, heading, sum_dx, sum_dy); sectors: 0 = E, then
clockwise (SE, S, SW, W, NW, N, NE)."""
import functools

import numpy as np

import mvtrim_amd as m

import blob_planes as bp
import blobs_inputs as bi
import headings_model as hm
import objects_inputs as oi
from derived_edge_inputs import MI355X_LDS, frozen, voters

TABLE_BYTES = 56                                  # MT_HEADING_TABLE_BYTES: 8 bins, a count, a pad word, two 64-bit sums
NONE = hm.NONE
E, SE, S, SW, W, NW, N, NE = range(8)


def with_threshold(p, thr):
    return m.ScanParams(float(thr), p.block_shift, p.clusters_needed, p.vertical_margin, p.vectors_needed, p.grid_w, p.grid_h)


def motion_of(rows, k):
    """[(n, records, heading, sum_dx, sum_dy)] -> HEADING_DTYPE [k], empty entries behind them."""
    mo = hm.empty_motion(k)
    for j, (n, rec, head, sx, sy) in enumerate(rows[:k]):
        mo["n"][j], mo["records"][j], mo["heading"][j], mo["sum_dx"][j], mo["sum_dy"][j] = n, rec, head, sx, sy
    return mo


# ------------------------------------------------------------------ 1. three blobs on the smallest grid, by hand

HAND_GW, HAND_GH, HAND_MARGIN = bp.GRIDS["63x12"].gw, bp.GRIDS["63x12"].gh, 1
# (cell x, cell y, votes, dx, dy): the blobs of objects_inputs.hand_case — A, B and C —
HAND_RECORDS = [
    (10, 2, 2, 7, 0), (11, 2, 1, 5, 1), (10, 3, 1, 12, 5),      # A: all E ((12, 5) lies on the boundary: the axis sector)
    (3, 6, 1, -6, 0), (4, 6, 1, -8, 2), (5, 6, 2, 5, -5),       # B: W, W, NE, NE — a 2 : 2 tie, the lower sector wins
    (20, 9, 1, 0, 0), (21, 9, 1, 0, 0),                         # C: still; it exists only where the threshold is 0
    # and, around them, records that belong to no entry:
    (4, 6, 1, 3, 0),                                            # |d|^2 = 9 inside a cell of B: below the threshold of 16
    (0, 2, 1, 5, 0),                                            # an active cell of column 0: never a centre
    (30, 4, 1, 5, 0),                                           # an isolated active cell: no centre
    (40, 0, 1, 5, 0),                                           # a margin row
    (63, 5, 1, 5, 0),                                           # out of bounds: column gw
]
_A = ([4, 0, 0, 0, 0, 0, 0, 0], 4, E, 7 + 7 + 5 + 12, 0 + 0 + 1 + 5)
_B16 = ([0, 0, 0, 0, 2, 0, 0, 2], 4, W, -6 - 8 + 5 + 5, 0 + 2 - 5 - 5)
_B0 = ([1, 0, 0, 0, 2, 0, 0, 2], 5, W, -6 - 8 + 5 + 5 + 3, 0 + 2 - 5 - 5)     # the slow record counts at threshold 0
_C0 = ([0] * 8, 2, NONE, 0, 0)
# threshold -> (centres, blobs, list entries, motion entries) of the full frame
HAND = {16: (6, 2, oi.HAND_LIST[:2], [_A, _B16]), 0: (8, 3, oi.HAND_LIST, [_A, _B0, _C0])}
# (threshold, allow byte, min_blob_cells) -> allowed of the full frame
HAND_ALLOWED = {(16, 0xFF, 1): 2, (0, 0xFF, 1): 3, (16, 1 << E, 1): 1, (0, 1 << E, 1): 2, (16, 1 << W, 1): 1, (0, 1 << W, 1): 2,
                (16, 0, 1): 0, (0, 0, 1): 1, (0, 0, 3): 0, (0, 0xFF, 3): 2, (16, 1 << NE, 1): 0, (0, 0xFF & ~(1 << W), 1): 2}


@functools.lru_cache(maxsize=None)
def hand_case(thr):
    """63 x 12, margin 1, threshold 16 or 0, four frames: 0 the full frame; 1 without side data; 2 with side data and no
    record; 3 the full frame again.  soff (0, 3) with one all-ones plane: under the mask frame 3 lies behind the last
    stream.  -> (params, mv, off, sd, soff, keeps)."""
    p = with_threshold(bi.grid(HAND_GW, HAND_GH, HAND_MARGIN), thr)
    full = voters(HAND_RECORDS)
    mv, off, sd = bi.batch_of([full, None, np.zeros(0, dtype=m.MV_DTYPE), full], 61)
    assert sd.tolist() == [1, 0, 1, 1]
    keeps = np.ones((1, HAND_GH, HAND_GW), dtype=bool)
    return (p, mv, off, sd) + frozen(np.array([0, 3], dtype=np.uint64), keeps)


def hand_want(thr, k, min_blob_cells=1, allow=0xFF, masked=False):
    """The dict headings_model.model_batch returns for hand_case(thr), from the numbers above."""
    centres, blobs, lst, mot = HAND[thr]
    full = [True, False, False, not masked]
    objs = sum(1 for e in lst if e[0] >= max(1, min_blob_cells))
    out = {"centres": np.array([centres * f for f in full], dtype=np.uint32), "blobs": np.array([blobs * f for f in full], dtype=np.uint32),
           "objects": np.array([objs * f for f in full], dtype=np.uint32),
           "list": np.stack([oi.om.entries(lst if f else [], k) for f in full]),
           "motion": np.stack([motion_of(mot if f else [], k) for f in full])}
    if (thr, allow, min_blob_cells) in HAND_ALLOWED:
        n = sum(1 for j, e in enumerate(lst[:k]) if e[0] >= max(1, min_blob_cells) and
                (mot[j][2] == NONE or (allow >> mot[j][2]) & 1))
        assert k < len(lst) or n == HAND_ALLOWED[(thr, allow, min_blob_cells)]
        out["allowed"] = np.array([n * f for f in full], dtype=np.uint32)
    return out


# ------------------------------------------------------------------ 2. seventeen blobs: k = 1, 2, 15, 16

@functools.lru_cache(maxsize=None)
def seventeen_case():
    """120 x 68, margin 3, one frame: blob i < 17 is a run of 18 - i cells on row 5 + 3 * i from column 10, every cell
    with one record of sector i & 7 — (dx, dy) = 6 * the sector's unit step — so rank i is blob i and the blob of rank 16
    is listed at no k.  -> (params, mv, off, sd)."""
    p = bi.grid(120, 68, margin=3)
    step = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)]
    cells = [(10 + j, 5 + 3 * i, 1) + step[i & 7] for i in range(17) for j in range(18 - i)]
    mv, off, sd = bi.batch_of([voters(cells)], 62)
    return (p,) + frozen(mv, off, sd)


def seventeen_motion(k):
    rows = []
    for i in range(16):
        n = [0] * 8
        n[i & 7] = 18 - i
        dx, dy = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)][i & 7]
        rows.append((n, 18 - i, i & 7, dx * (18 - i), dy * (18 - i)))
    return motion_of(rows, k)[None]


# ------------------------------------------------------------------ 3. word seams, a direction per blob

SEAM_DIRS = {300: (0, -2), 1000: (-2, 0), 120: (2, 2), 60: (1, 0)}        # by the bar's first column: N, W, SE, E


@functools.lru_cache(maxsize=None)
def seams_case():
    """objects_inputs.seams_case's plane (2000 x 9, two-pixel cells: bars across the column-64, 128 and 1024 seams and a
    blob of 38 cells) with a direction per blob and threshold 1.  hand: the four motion entries in list order."""
    c = oi.seams_case()
    p = with_threshold(c.p, 1.0)
    cells = []
    for x, y, n in oi.SEAM_BARS + oi.SEAM_BIG:
        cells += [(x + i, y, 1) + SEAM_DIRS[x] for i in range(n)]
    mv, off, sd = bi.batch_of([voters(cells, p.block_shift)], 63)
    hand = [([0, 0, 0, 0, 0, 0, 38, 0], 38, N, 0, -76), ([0, 0, 0, 0, 31, 0, 0, 0], 31, W, -62, 0),
            ([0, 16, 0, 0, 0, 0, 0, 0], 16, SE, 32, 32), ([11, 0, 0, 0, 0, 0, 0, 0], 11, E, 11, 0)]
    return (p,) + frozen(mv, off, sd) + (hand,)


# ------------------------------------------------------------------ 4. one frame of 40 000 records

BIG_RECORDS, BIG_DX = 40000, 65535


BIG_GW, BIG_GH = 2050, 4


@functools.lru_cache(maxsize=None)
def big_case():
    """2050 x 4 cells of 16 pixels, margin 0, two frames.  Frame 0 holds three slow records, so that frame 1's 40-byte
    records begin at byte 120 of the array: 8-byte aligned, not 128-byte aligned.  Frame 1 holds 40 000 records with
    src_x = -32768 and dst_x = 32767 — dx = 65535, the largest there is — half of them in cell (2047, 1) and half in
    (2047, 2): one blob of two cells (column 2047 is gw - 3).  -> (params, mv, off, sd); by hand: the list entry
    (2, 2050 + 2047, 2047, 1, 2047, 2) and the motion entry n[E] = records = 40 000, sum_dx = 40 000 * 65 535, sum_dy = 0."""
    p = m.ScanParams.from_config(16 * BIG_GW, 16 * BIG_GH, vertical_mask=0.0, vectors_needed=1, clusters_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (BIG_GW, BIG_GH, 0, 4)
    mv = np.zeros(3 + BIG_RECORDS, dtype=m.MV_DTYPE)
    mv["dst_x"][:3], mv["dst_y"][:3], mv["src_x"][:3], mv["src_y"][:3] = 100, 20, 99, 20
    mv["src_x"][3:], mv["dst_x"][3:] = -32768, 32767
    mv["dst_y"][3::2], mv["dst_y"][4::2] = 24, 40
    mv["src_y"][3:] = mv["dst_y"][3:]
    off = np.array([0, 3, 3 + BIG_RECORDS], dtype=np.uint64)
    return (p,) + frozen(mv, off, np.ones(2, dtype=np.uint8))


BIG_LIST = (2, BIG_GW + 2047, 2047, 1, 2047, 2)
BIG_MOTION = ([BIG_RECORDS, 0, 0, 0, 0, 0, 0, 0], BIG_RECORDS, E, BIG_RECORDS * BIG_DX, 0)


# ------------------------------------------------------------------ 5. the cliff

def lds_by_hand(gw, R, k):
    """csrc/headings_kernels.h: the object scan's layout and, behind it, k entries of the motion table."""
    return oi.lds_by_hand(gw, R, k) + k * TABLE_BYTES


def preview_or_none(p, k, lds=MI355X_LDS):
    from mvtrim_amd import headings
    try:
        return headings.preview(p, k, lds)
    except m.MtgpuError as e:
        if e.code != m._abi.MT_ERR_UNSUPPORTED:
            raise
        return None


@functools.lru_cache(maxsize=None)
def cliff_rows(k):
    """The tallest 65-column grid mtgpu_headings_preview accepts for k entries at 163 840 bytes, by bisection."""
    return bi._largest(lambda gh: preview_or_none(bi.limit_params(oi.CLIFF_GW, gh), k) is not None, 16383)


@functools.lru_cache(maxsize=None)
def cliff_case(k):
    """65 x cliff_rows(k), margin 0, one frame: twenty runs of 2 .. 21 cells on every second row upwards from the LAST
    row — the labels and the centre words at the end of the layout — run i moving in sector i & 7."""
    gh = cliff_rows(k)
    p = bi.limit_params(oi.CLIFF_GW, gh, vectors_needed=1, clusters_needed=1)
    step = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)]
    cells = [(1 + i + j, gh - 1 - 2 * i, 1) + step[i & 7] for i in range(20) for j in range(2 + i)]
    mv, off, sd = bi.batch_of([voters(cells, p.block_shift)], 64)
    return (p,) + frozen(mv, off, sd)


# ------------------------------------------------------------------ 6. random draws

def random_case(seed):
    """A small random grid and batch: 6 frames of clustered records with random displacements (a fifth of them still, a
    fifth slow), one frame without side data, one without a record; a random keep plane per stream for the masked run.
    -> (params, mv, off, sd, soff, keeps)."""
    rng = np.random.RandomState(7000 + seed)
    gw, gh = int(rng.randint(5, 140)), int(rng.randint(4, 40))
    margin = int(rng.randint(0, 2)) if gh > 6 else 0
    p = with_threshold(bi.grid(gw, gh, margin, vn=int(rng.randint(1, 3))), [0.0, 4.0, 16.0][seed % 3])
    frames = []
    for f in range(8):
        if f == 3:
            frames.append(None)
            continue
        if f == 5:
            frames.append(np.zeros(0, dtype=m.MV_DTYPE))
            continue
        nb = int(rng.randint(1, 24))
        recs = []
        for _ in range(nb):
            x0, y0 = int(rng.randint(0, gw)), int(rng.randint(0, gh))
            w, h = int(rng.randint(1, 6)), int(rng.randint(1, 4))
            ddx, ddy = (int(v) for v in rng.randint(-9, 10, size=2))
            for y in range(y0, min(y0 + h, gh)):
                for x in range(x0, min(x0 + w, gw)):
                    for _ in range(int(rng.randint(1, 4))):
                        kind = rng.randint(0, 5)
                        d = (0, 0) if kind == 0 else (1, 0) if kind == 1 else (ddx + int(rng.randint(-2, 3)), ddy + int(rng.randint(-2, 3)))
                        recs.append((x, y, 1) + d)
        frames.append(voters(recs))
    mv, off, sd = bi.batch_of(frames, 7100 + seed)
    soff = np.array([0, 3, 3, 8], dtype=np.uint64)
    keeps = rng.rand(3, gh, gw) >= 0.15
    return (p,) + frozen(mv, off, sd, soff, keeps)
