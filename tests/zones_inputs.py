"""Inputs of tests/test_gpu_zones.py (the masked centre scan, include/mtgpu_zones.h) with the values derived BY HAND from
their construction, the ten-line numpy restatement of the AND rule, and the record filter that lets the unchanged
oracle supply expected values for vectors_needed >= 1.  tests/test_zones_host.py checks all of it against the oracle
without a GPU.  Everything is built once per process and handed out read-only."""
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import zones

import oracle_binding as ob
from derived_edge_inputs import frozen, voters
from scan_checks import junk_padding


# ------------------------------------------------------------------ the AND rule, restated

def zone_counts_np(p, mv, keep):
    """(centres under the mask, centres without it) of one frame WITH side data: active = votes >= vn AND (keep OR the
    row is not analysed); a centre is an active cell of an analysed row, x in [1, gw - 2], with an active 4-neighbour."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    d2 = (mv["dst_x"].astype(np.int64) - mv["src_x"]) ** 2 + (mv["dst_y"].astype(np.int64) - mv["src_y"]) ** 2
    gx, gy = mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift
    ok = ~(d2.astype(np.float64) < p.mv_threshold_sq) & (gx >= 0) & (gx < gw) & (gy >= 0) & (gy < gh)
    ok &= rows[np.clip(gy, 0, gh - 1), 0]
    votes = np.zeros((gh, gw), dtype=np.int64)
    np.add.at(votes, (gy[ok], gx[ok]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)

    def count(a):
        z = np.pad(a, 1)
        nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
        return int((a & nb & rows)[:, 1:gw - 1].sum())
    return count(act & (np.asarray(keep, dtype=bool) | ~rows)), count(act)


def has_side_data(off, sd):
    return np.asarray(sd).astype(bool) if sd is not None else np.diff(np.asarray(off).astype(np.int64)) > 0


def stream_of_frames(soff, n_frames):
    """Stream index per frame; len(soff) - 1 for a frame at or past soff[-1]."""
    return np.searchsorted(np.asarray(soff).astype(np.int64), np.arange(n_frames), side="right") - 1


def model_batch(p, mv, off, sd, soff, keeps):
    """(centres, centres_all) uint32 [F] of a batch from zone_counts_np; keeps: bool [S, gh, gw]."""
    F = len(off) - 1
    has, st = has_side_data(off, sd), stream_of_frames(soff, F)
    c, ca = np.zeros(F, dtype=np.uint32), np.zeros(F, dtype=np.uint32)
    for f in range(F):
        if has[f] and 0 <= st[f] < len(keeps):
            c[f], ca[f] = zone_counts_np(p, mv[int(off[f]):int(off[f + 1])], keeps[st[f]])
    return c, ca


def filter_records(p, mv, off, soff, keeps):
    """(mv, off) with every record removed whose destination cell (dst_x >> shift, dst_y >> shift) lies in the grid and
    is ignored by its frame's stream.  A frame behind the last stream loses every record."""
    F = len(off) - 1
    fr = np.repeat(np.arange(F), np.diff(np.asarray(off).astype(np.int64)))
    mv = mv[int(off[0]):int(off[-1])]
    st = stream_of_frames(soff, F)[fr]
    gx, gy = mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift
    inside = (gx >= 0) & (gx < p.grid_w) & (gy >= 0) & (gy < p.grid_h)
    live = (st >= 0) & (st < len(keeps))
    kept = np.asarray(keeps, dtype=bool)[np.clip(st, 0, len(keeps) - 1), np.clip(gy, 0, p.grid_h - 1), np.clip(gx, 0, p.grid_w - 1)]
    take = live & (~inside | kept)
    new_off = np.concatenate([[0], np.cumsum(np.bincount(fr[take], minlength=F))]).astype(np.uint64)
    return np.ascontiguousarray(mv[take]), new_off


def oracle_batch(p, mv, off, sd, soff, keeps):
    """(flags, centres, centres_all) for vectors_needed >= 1: the unchanged oracle on the filtered records, has_sd passed
    explicitly and unchanged; centres_all: the oracle on the records as they are.  Frames behind the last stream: 0."""
    assert (p.vectors_needed & 0xFF) >= 1
    has = has_side_data(off, sd).astype(np.uint8)
    behind = stream_of_frames(soff, len(off) - 1) >= len(keeps)
    fmv, foff = filter_records(p, mv, off, soff, keeps)
    fl, ce = ob.scan_centres(p, fmv, foff, has, nthreads=4)
    ca = ob.scan_centres(p, mv, off, has, nthreads=4)[1].copy()
    ca[behind] = 0
    return fl, ce, ca


def pack_keeps(keeps):
    return np.ascontiguousarray(np.stack([zones.pack_keep(k) for k in keeps]))


# ------------------------------------------------------------------ 2. random masks

# (width, height, vertical_mask, vectors_needed): grid widths before, at and behind one and two mask words with six
# rows, margin 0 and 1; the 1080p and 4K grids (4 frames each).
RANDOM_CASES = [
    (1008, 96, 0.0, 1), (1008, 96, 0.2, 2), (1024, 96, 0.0, 2), (1024, 96, 0.2, 3), (1040, 96, 0.0, 3), (1040, 96, 0.2, 1),
    (2048, 96, 0.0, 1), (2048, 96, 0.2, 3), (2064, 96, 0.0, 2), (2064, 96, 0.2, 1),
    (1920, 1080, 0.05, 2), (1920, 1080, 0.0, 3), (3840, 2160, 0.05, 1), (3840, 2160, 0.0, 2),
]
RANDOM_GRIDS = {1008: 63, 1024: 64, 1040: 65, 2048: 128, 2064: 129, 1920: 120, 3840: 240}


def clustered_frame(rng, p, n_blobs):
    """Blobs of 2 x 2 or 3 x 2 neighbouring cells with 1 .. 4 votes each (|d|^2 = 25), anywhere in the grid, and a few
    records that pass no threshold or lie outside the grid."""
    cells = []
    for _ in range(n_blobs):
        x0, y0 = rng.randint(0, max(p.grid_w - 2, 1)), rng.randint(0, max(p.grid_h - 1, 1))
        for dx in range(2 + rng.randint(0, 2)):
            for dy in range(2):
                if x0 + dx < p.grid_w and y0 + dy < p.grid_h:
                    cells.append((x0 + dx, y0 + dy, int(rng.randint(1, 5)), 5, 0))
    still = voters([(int(rng.randint(0, p.grid_w)), int(rng.randint(0, p.grid_h)), 3, 1, 1)], p.block_shift)
    out = voters([(p.grid_w + 1, 1, 2, 5, 0), (2, p.grid_h + 2, 2, 5, 0)], p.block_shift)
    mv = np.concatenate([voters(cells, p.block_shift), still, out])
    return mv[rng.permutation(len(mv))]


@functools.lru_cache(maxsize=None)
def random_case(i):
    """(params, mv, off, sd, soff, keeps bool [5, gh, gw]).  Streams: 0, 2 and 4 with masks of their own (30 % of the
    cells cleared), 1 empty, 3 with an all-zero mask.  Small grids: 12 frames, frames 2, 6 and 9 carry records and have
    has_sd == 0; 1080p and 4K: 4 frames."""
    width, height, vmask, vn = RANDOM_CASES[i]
    p = m.ScanParams.from_config(width, height, vertical_mask=vmask, vectors_needed=vn, clusters_needed=2)
    assert p.grid_w == RANDOM_GRIDS[width]
    rng = np.random.RandomState(1000 + i)
    big = width in (1920, 3840)
    F = 4 if big else 12
    frames = [clustered_frame(rng, p, (40 if big else 8) + 4 * (f % 3)) for f in range(F)]
    b = m.FrameBatch.from_frames(frames)
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    sd = np.ones(F, dtype=np.uint8)
    if not big:
        sd[[2, 6, 9]] = 0
    soff = np.array([0, 1, 1, 2, 3, 4] if big else [0, 4, 4, 8, 10, 12], dtype=np.uint64)
    keeps = rng.rand(5, p.grid_h, p.grid_w) >= 0.3
    keeps[3] = False
    return (p,) + frozen(mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), sd, soff, keeps)


# ------------------------------------------------------------------ 3. word seams, by hand

SEAM_W, SEAM_H = 2080, 64          # 130 x 4 cells, W = 3
SEAM_KW = dict(vertical_mask=0.0, vectors_needed=1, clusters_needed=1)
# Frame A: runs x = 62 .. 65 and x = 126 .. 129 on row 0, a vertical pair (20, 2) + (20, 3).  Column 129 is the last
# one: never a centre.  Unmasked: 4 + 3 + 2 = 9.
# Frame B: the pairs (63, 64) on row 0 and (127, 128) on row 2, each across a word boundary: 2 + 2 = 4.  With one cell
# of a pair ignored the other one has no neighbour left: a carry taken from the UNMASKED neighbour word would count it.
SEAM_CLEARED = [None, (63, 0), (64, 0), (127, 0), (128, 0), (20, 2), (20, 3)]
#   mask           frame A                                                            frame B
#   full           9                                                                  4
#   (63, 0)        62 alone 0; 64, 65: 2; second run 3; pair 2          = 7           64 alone: 0; (127, 128): 2   = 2
#   (64, 0)        62, 63: 2; 65 alone 0; 3; 2                          = 7           63 alone: 0; 2               = 2
#   (127, 0)       4; 126 alone 0; 128 (129 active, last column): 1; 2  = 7           row 0 clears nothing on row 2 = 4
#   (128, 0)       4; 126, 127: 2; 129 alone, last column: 0; 2         = 8           4
#   (20, 2)        4; 3; (20, 3) alone: 0                               = 7           4
#   (20, 3)        4; 3; (20, 2) alone: 0                               = 7           4
SEAM_HAND = [(9, 4), (7, 2), (7, 2), (7, 4), (8, 4), (7, 4), (7, 4)]
SEAM_HAND_ALL = (9, 4)


@functools.lru_cache(maxsize=None)
def seam_case():
    """(params, mv, off, sd, soff, keeps, hand centres [14], hand centres_all [14]): seven streams — the full mask and
    the six single cleared cells — of frames A and B each."""
    p = m.ScanParams.from_config(SEAM_W, SEAM_H, **SEAM_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (130, 4, 0)
    a = voters([(x, 0, 1, 5, 0) for x in (62, 63, 64, 65, 126, 127, 128, 129)] + [(20, 2, 1, 5, 0), (20, 3, 1, 5, 0)])
    b = voters([(63, 0, 1, 5, 0), (64, 0, 1, 5, 0), (127, 2, 1, 5, 0), (128, 2, 1, 5, 0)])
    batch = m.FrameBatch.from_frames([a, b] * len(SEAM_CLEARED))
    keeps = np.ones((len(SEAM_CLEARED), 4, 130), dtype=bool)
    for s, cell in enumerate(SEAM_CLEARED):
        if cell:
            keeps[s, cell[1], cell[0]] = False
    soff = np.arange(len(SEAM_CLEARED) + 1, dtype=np.uint64) * 2
    hand = np.array([v for pair in SEAM_HAND for v in pair], dtype=np.uint32)
    hand_all = np.array(list(SEAM_HAND_ALL) * len(SEAM_CLEARED), dtype=np.uint32)
    return (p,) + frozen(np.ascontiguousarray(batch.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(batch.frame_off, dtype=np.uint64),
                         np.ones(2 * len(SEAM_CLEARED), dtype=np.uint8), soff, keeps, hand, hand_all)


# ------------------------------------------------------------------ 4. vectors_needed == 0, by hand

VN0_W, VN0_H = 160, 128            # 10 x 8 cells


def _only(cells):
    k = np.zeros((8, 10), dtype=bool)
    for x, y in cells:
        k[y, x] = True
    return k


@functools.lru_cache(maxsize=None)
def vn0_case(margin):
    """(params, off, sd, soff, keeps, hand centres, hand centres_all): one frame with side data and NO record per mask,
    one stream per mask.  vn == 0: every kept analysed cell is active; with margin 1 rows 0 and 7 are active neighbours.
      margin 0                                                          margin 1 (analysed rows 1 .. 6)
      full          8 rows x columns 1 .. 8                    = 64     6 x 8                                       = 48
      checkerboard  (x + y even) no kept cell has a kept               row 1: x = 1, 3, 5, 7 and row 6: x = 2, 4, 6, 8
                    4-neighbour                                =  0     have the margin row as neighbour            =  8
      (4,3)+(5,3)   both centres                               =  2     the same                                    =  2
      (0,3)+(1,3)   column 0 is never a centre                 =  1     the same                                    =  1
      (4,1)+(5,1)   both centres                               =  2     first analysed row: the same                =  2
      (4,1)         alone                                      =  0     the margin row (4, 0) is an active neighbour =  1
      (4,0)         alone; the row outside the grid: inactive  =  0     row 0 is not analysed: the bit has no effect, and
                                                                        no analysed cell is kept                    =  0"""
    p = m.ScanParams.from_config(VN0_W, VN0_H, vertical_mask=0.125 * margin, vectors_needed=0, clusters_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.vectors_needed) == (10, 8, margin, 0)
    yy, xx = np.mgrid[0:8, 0:10]
    keeps = np.stack([np.ones((8, 10), dtype=bool), (xx + yy) % 2 == 0, _only([(4, 3), (5, 3)]), _only([(0, 3), (1, 3)]),
                      _only([(4, 1), (5, 1)]), _only([(4, 1)]), _only([(4, 0)])])
    hand = np.array([64, 0, 2, 1, 2, 0, 0] if margin == 0 else [48, 8, 2, 1, 2, 1, 0], dtype=np.uint32)
    n = len(keeps)
    hand_all = np.full(n, 64 if margin == 0 else 48, dtype=np.uint32)
    return (p,) + frozen(np.zeros(n + 1, dtype=np.uint64), np.ones(n, dtype=np.uint8), np.arange(n + 1, dtype=np.uint64), keeps,
                         hand, hand_all)


# ------------------------------------------------------------------ 6. the stream lookup, by hand

LOOKUP_W, LOOKUP_H = 1280, 96      # 80 x 6 cells
LOOKUP_SOFF = [0, 0, 1, 3, 3, 6, 7]           # six streams of 0, 1, 2, 0, 3 and 1 frames
LOOKUP_SD = [1, 1, 1, 0, 1, 1, 1]             # frame 3, the first of stream 4, is a key frame without side data
# Band s = columns [2 + 12 s, 14 + 12 s); every frame holds, in band s, a run of s + 2 active cells on row 2 from column
# 3 + 12 s (band 5: 63 .. 69, across a word boundary).  Every cell of a run is a centre (no run touches column 0 or
# 79), runs are at least five columns apart.  Stream s keeps band s only: its frames count s + 2.
LOOKUP_HAND = [3, 4, 4, 0, 6, 6, 7]
LOOKUP_HAND_ALL = [27, 27, 27, 0, 27, 27, 27]          # 2 + 3 + 4 + 5 + 6 + 7
LOOKUP_EXTRA = 2                                       # frames behind stream_off[n_streams] on the device entry point


@functools.lru_cache(maxsize=None)
def lookup_case():
    """(params, mv, off, sd, soff, keeps, hand, hand_all) with 7 + LOOKUP_EXTRA frames of the same records; the host
    entry point takes the first 7."""
    p = m.ScanParams.from_config(LOOKUP_W, LOOKUP_H, vertical_mask=0.0, vectors_needed=1, clusters_needed=4)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (80, 6, 0)
    one = voters([(3 + 12 * s + j, 2, 1, 5, 0) for s in range(6) for j in range(s + 2)])
    F = 7 + LOOKUP_EXTRA
    b = m.FrameBatch.from_frames([one] * F)
    keeps = np.zeros((6, 6, 80), dtype=bool)
    for s in range(6):
        keeps[s, :, 2 + 12 * s:14 + 12 * s] = True
    sd = np.array(LOOKUP_SD + [1] * LOOKUP_EXTRA, dtype=np.uint8)
    hand = np.array(LOOKUP_HAND + [0] * LOOKUP_EXTRA, dtype=np.uint32)
    hand_all = np.array(LOOKUP_HAND_ALL + [0] * LOOKUP_EXTRA, dtype=np.uint32)
    return (p,) + frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64), sd,
                         np.array(LOOKUP_SOFF, dtype=np.uint64), keeps, hand, hand_all)


# ------------------------------------------------------------------ 8. two-kernel planning

PLAN_FRAMES = 40000                # more than 32 planning blocks of 1024 frames: the count kernel and the scatter kernel


@functools.lru_cache(maxsize=None)
def plan_case():
    """(params, mv, off, sd, soff, keeps): 40 000 frames of 4 records — a horizontal pair and a vertical pair of cells,
    one vote each, on the 65 x 6 grid (vn 1: two centres per pair unless the mask takes a cell); every 7th frame has no
    side data; two streams with random masks (30 % cleared)."""
    p = m.ScanParams.from_config(1040, 96, vertical_mask=0.0, vectors_needed=1, clusters_needed=3)
    assert (p.grid_w, p.grid_h) == (65, 6)
    f = np.arange(PLAN_FRAMES, dtype=np.int64)
    xa, ya = 1 + (f * 7) % 62, (f * 5) % 6
    xb, yb = 1 + (f * 11 + 30) % 63, (f * 3) % 5
    gx = np.stack([xa, xa + 1, xb, xb], axis=1).reshape(-1)
    gy = np.stack([ya, ya, yb, yb + 1], axis=1).reshape(-1)
    mv = np.zeros(4 * PLAN_FRAMES, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = gx * 16 + 8, gy * 16 + 8
    mv["src_x"], mv["src_y"] = gx * 16 + 3, gy * 16 + 8
    sd = np.ones(PLAN_FRAMES, dtype=np.uint8)
    sd[::7] = 0
    keeps = np.random.RandomState(8).rand(2, 6, 65) >= 0.3
    return (p,) + frozen(mv, np.arange(PLAN_FRAMES + 1, dtype=np.uint64) * 4, sd, np.array([0, 17001, PLAN_FRAMES], dtype=np.uint64),
                         keeps)


# ------------------------------------------------------------------ 5. the margin as a mask

MARGIN_MASKS = ((0.05, 3), (0.10, 6))          # VERTICAL_MASK -> margin rows of the 68-row grid


@functools.lru_cache(maxsize=None)
def margin_case():
    """(mv, off, sd): 24 random 1080p frames of synth.random_frames — whose motion rarely reaches the outer rows — each
    with 30 blobs of clustered_frame added, which fall on every row of the grid, the strips included."""
    from mvtrim_amd import synth
    rng = np.random.RandomState(50)
    mv, off, sd = synth.random_frames(rng, 24, 3000, 1920, 1080)
    p0 = m.ScanParams.from_config(1920, 1080, vertical_mask=0.0)
    frames = [np.concatenate([mv[int(off[f]):int(off[f + 1])], clustered_frame(rng, p0, 30)]) for f in range(24)]
    b = m.FrameBatch.from_frames(frames)
    out = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(out, rng)
    return frozen(out, np.ascontiguousarray(b.frame_off, dtype=np.uint64), np.ones(24, dtype=np.uint8))


# ------------------------------------------------------------------ what every parity input has to hold

def counts_to_count(c, ca, off, sd):
    """The condition on a parity input: of the frames with side data and records, at least half have a non-zero masked
    count and at least a quarter lose centres to the mask.  A parity test on all-zero counts shows nothing."""
    take = has_side_data(off, sd) & (np.diff(np.asarray(off).astype(np.int64)) > 0)
    n = int(take.sum())
    return n > 0 and 2 * int((c[take] > 0).sum()) >= n and 4 * int((ca[take] > c[take]).sum()) >= n
