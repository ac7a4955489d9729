"""Inputs of tests/test_gpu_blobs.py (the blob scan, include/mtgpu_blobs.h) with the values derived BY HAND from their
construction.  tests/test_blobs_host.py holds every hand value against the numpy restatement (tests/blobs_model.py)
without a GPU.  Everything is built once per process and handed out read-only.

A case is a Case tuple: params, mv, off, sd, soff / keeps (bool [S, gh, gw]; both None: no mask) and `hand`, a dict of
per-frame lists "centres", "blobs", "largest", "box" ((x0, y0, x1, y1), inclusive; NO_BOX without a blob).  Every active
cell of a shape gets one vote of |d|^2 = 25 under VECTORS_NEEDED 1 and CLUSTERS_NEEDED 1, unless the case says otherwise."""
import collections
import functools

import numpy as np

import mvtrim_amd as m

import zones_inputs as zi
from blobs_model import NO_BOX
from derived_edge_inputs import MI355X_LDS, frozen, voters
from scan_checks import junk_padding

Case = collections.namedtuple("Case", "p mv off sd soff keeps hand")


def grid(gw, gh, margin=0, vn=1, cn=1):
    """The context of a gw x gh grid of 16-pixel cells with `margin` rows masked at the top and at the bottom."""
    p = m.ScanParams.from_config(16 * gw, 16 * gh, vertical_mask=(margin + 0.5) / gh if margin else 0.0, vectors_needed=vn,
                                 clusters_needed=cn)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (gw, gh, margin, 4)
    return p


def cells_frame(cells):
    return voters([(x, y, 1, 5, 0) for x, y in cells])


def batch_of(frames, seed, sd=None):
    """Frames (record arrays, None: no side data and no record) -> (mv, off, sd); records shuffled, junk in the padding."""
    rng = np.random.RandomState(seed)
    b = m.FrameBatch.from_frames([None if f is None else f[rng.permutation(len(f))] for f in frames])
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    has = np.ascontiguousarray(b.has_sd, dtype=np.uint8) if sd is None else np.array(sd, dtype=np.uint8)
    return frozen(mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), has)


def hand_of(rows):
    """[(centres, blobs, largest, box)] per frame -> the dict of lists."""
    return {"centres": [r[0] for r in rows], "blobs": [r[1] for r in rows], "largest": [r[2] for r in rows],
            "box": [tuple(r[3]) for r in rows]}


def only(gw, gh, cells):
    k = np.zeros((gh, gw), dtype=bool)
    for x, y in cells:
        k[y, x] = True
    return k


# ------------------------------------------------------------------ 1. centre cells only

@functools.lru_cache(maxsize=None)
def edge_columns_case():
    """8 x 6, margin 0.  Frame 0: column 0 active on rows 1 .. 3, column 1 on rows 1 and 3.  (1, 1) and (1, 3) are
    centres (their neighbour in column 0 is active); column 0 never is; (1, 2) is not active.  The two centres touch only
    through (0, 2), a non-centre: 2 centres, 2 blobs of 1 cell; the tie goes to (1, 1).  Frame 1: the mirror image at
    column gw - 1 = 7."""
    p = grid(8, 6)
    left = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 3)]
    right = [(7 - x, y) for x, y in left]
    mv, off, sd = batch_of([cells_frame(left), cells_frame(right)], 1)
    return Case(p, mv, off, sd, None, None, hand_of([(2, 2, 1, (1, 1, 1, 1)), (2, 2, 1, (6, 1, 6, 1))]))


@functools.lru_cache(maxsize=None)
def halo_row_case():
    """8 x 8, margin 1 (analysed rows 1 .. 6), VECTORS_NEEDED 0, frames with side data and no record, one stream per mask.
    vn == 0: every cell of halo rows 0 and 7 is active, an analysed cell is active iff kept.
      stream 0  keeps (2, 1) and (4, 1): each has its halo-row cell above as an active neighbour, so both are centres;
                (3, 1) is ignored; they touch only through (2, 0) .. (4, 0), halo cells, which are no centres: 2 blobs of 1.
      stream 1  keeps (2, 6) and (3, 6), the last analysed row: one blob of 2.
      stream 2  keeps (0, 3), (1, 3) and (6, 3), (7, 3): (1, 3) and (6, 3) are centres, the edge columns are not: 2 blobs
                of 1, the tie goes to (1, 3)."""
    p = grid(8, 8, margin=1, vn=0)
    keeps = np.stack([only(8, 8, [(2, 1), (4, 1)]), only(8, 8, [(2, 6), (3, 6)]), only(8, 8, [(0, 3), (1, 3), (6, 3), (7, 3)])])
    off, sd, soff = np.zeros(4, dtype=np.uint64), np.ones(3, dtype=np.uint8), np.arange(4, dtype=np.uint64)
    hand = hand_of([(2, 2, 1, (2, 1, 2, 1)), (2, 1, 2, (2, 6, 3, 6)), (2, 2, 1, (1, 3, 1, 3))])
    return Case(p, np.zeros(0, dtype=m.MV_DTYPE), *frozen(off, sd, soff, keeps), hand)


# ------------------------------------------------------------------ 2. word seams

SEAM_GW = (65, 129, 130)
# gw -> the cells cleared, one per stream after the full mask, each next to a seam.  The bar: row 2, columns 60 .. gw - 1,
# all active; its centres are columns 60 .. gw - 2 (the last column never is one): gw - 61 cells, one blob.
#   65   bar 60 .. 64, centres 60 .. 63.   clear 62: {60, 61} and {63} (63's neighbour 64 lies across the seam): 2 blobs
#   129  centres 60 .. 127.                clear 63: {60 .. 62} and {64 .. 127}: 2 blobs, largest 64, box 64 .. 127
#                                          clear 64: {60 .. 63} and {65 .. 127}: 2 blobs, largest 63, box 65 .. 127
#   130  centres 60 .. 128.                clear 127: {60 .. 126} and {128} (neighbour 129): 2 blobs, largest 67
#                                          clear 128: {60 .. 127}; 129 is alone and in the last column: 1 blob of 68
#                                          clear 63: {60 .. 62} and {64 .. 128}: 2 blobs, largest 65, box 64 .. 128
SEAM_CUTS = {65: [62], 129: [63, 64], 130: [127, 128, 63]}
SEAM_HAND = {65: [(4, 1, 4, (60, 2, 63, 2)), (3, 2, 2, (60, 2, 61, 2))],
             129: [(68, 1, 68, (60, 2, 127, 2)), (67, 2, 64, (64, 2, 127, 2)), (67, 2, 63, (65, 2, 127, 2))],
             130: [(69, 1, 69, (60, 2, 128, 2)), (68, 2, 67, (60, 2, 126, 2)), (68, 1, 68, (60, 2, 127, 2)),
                   (68, 2, 65, (64, 2, 128, 2))]}


@functools.lru_cache(maxsize=None)
def seam_case(gw):
    """gw x 6, margin 0: the bar in every frame, stream 0 with the full mask, then one stream per cleared cell.  The same
    frames without a mask (soff / keeps dropped) read hand[0] everywhere: one blob again."""
    p = grid(gw, 6)
    cuts = SEAM_CUTS[gw]
    bar = cells_frame([(x, 2) for x in range(60, gw)])
    mv, off, sd = batch_of([bar] * (1 + len(cuts)), gw)
    keeps = np.ones((1 + len(cuts), 6, gw), dtype=bool)
    for s, x in enumerate(cuts):
        keeps[1 + s, 2, x] = False
    return Case(p, mv, off, sd, *frozen(np.arange(2 + len(cuts), dtype=np.uint64), keeps), hand_of(SEAM_HAND[gw]))


# ------------------------------------------------------------------ 3. late merges (20 x 12, margin 0)

def comb_cells():
    """Eight teeth, columns 2, 4, .. 16 on rows 1 .. 10, joined only on the last analysed row 11 (columns 2 .. 16):
    8 * 10 + 15 = 95 cells, one blob, box (2, 1) .. (16, 11)."""
    return [(x, y) for x in range(2, 17, 2) for y in range(1, 11)] + [(x, 11) for x in range(2, 17)]


def u_cells():
    """Columns 3 and 12 on rows 2 .. 9 and row 9 between them: 8 + 8 + 10 - 2 = 24 cells, box (3, 2) .. (12, 9)."""
    return sorted({(3, y) for y in range(2, 10)} | {(12, y) for y in range(2, 10)} | {(x, 9) for x in range(3, 13)})


def ring_cells():
    """Rows 2 and 9 on columns 4 .. 13 and columns 4 and 13 on rows 3 .. 8: 10 + 10 + 6 + 6 = 32 cells; inside it, apart,
    (8, 5), (9, 5), (8, 6): a second blob of 3."""
    ring = [(x, y) for y in (2, 9) for x in range(4, 14)] + [(x, y) for x in (4, 13) for y in range(3, 9)]
    return ring + [(8, 5), (9, 5), (8, 6)]


@functools.lru_cache(maxsize=None)
def late_merge_case():
    p = grid(20, 12)
    mv, off, sd = batch_of([cells_frame(comb_cells()), cells_frame(u_cells()), cells_frame(ring_cells())], 3)
    return Case(p, mv, off, sd, None, None, hand_of([(95, 1, 95, (2, 1, 16, 11)), (24, 1, 24, (3, 2, 12, 9)),
                                                     (35, 2, 32, (4, 2, 13, 9))]))


# ------------------------------------------------------------------ 4. thin and long

def serpentine_cells(gw, y_lo, y_hi):
    """Full rows (columns 1 .. gw - 2) on y_lo, y_lo + 2, .. joined at alternating ends by one cell on the rows between:
    one path; every cell has a neighbour on the path, so every cell is a centre."""
    cells, right = [], True
    full = list(range(y_lo, y_hi, 2))
    for i, y in enumerate(full):
        cells += [(x, y) for x in range(1, gw - 1)]
        if i + 1 < len(full):
            cells.append((gw - 2 if right else 1, y + 1))
            right = not right
    return cells, (1, full[0], gw - 2, full[-1])


def spiral_cells(x0, y0, x1, y1):
    """A square spiral inwards from (x0, y0), heading east, with one free cell between its turns: a step is taken only to a
    cell inside [x0, x1] x [y0, y1] whose only neighbour on the path is the cell the step comes from; where it cannot go
    straight on it turns right, and it ends when it cannot move after a turn.  Consecutive cells are neighbours and no
    two others are, so it is one thin path."""
    x, y, dx, dy = x0, y0, 1, 0
    cells, on = [(x, y)], {(x0, y0)}

    def free(cx, cy, ddx, ddy):
        nx, ny = cx + ddx, cy + ddy
        if not (x0 <= nx <= x1 and y0 <= ny <= y1) or (nx, ny) in on:
            return False
        return all((ax, ay) == (cx, cy) or (ax, ay) not in on for ax, ay in ((nx + 1, ny), (nx - 1, ny), (nx, ny + 1), (nx, ny - 1)))
    while True:
        if not free(x, y, dx, dy):
            dx, dy = -dy, dx
            if not free(x, y, dx, dy):
                break
        x, y = x + dx, y + dy
        cells.append((x, y))
        on.add((x, y))
    return cells


SERPENTINE_66 = 6 * 64 + 5         # 66 x 12, margin 0: full rows 0, 2, .. 10 of 64 cells and five joints


@functools.lru_cache(maxsize=None)
def serpentine_case(which):
    """"66x12": one frame, margin 0, path length 389, box (1, 0) .. (64, 10).  "4k": 240 x 135, margin 6 (the 4K grid),
    eight frames in one batch: full rows 6, 8, .. 128 (62 rows of 238) and 61 joints = 14 817 cells, box (1, 6) ..
    (238, 128).  "spiral": 120 x 68, margin 3 (the 1080p grid): the spiral over columns 1 .. 118, rows 3 .. 64."""
    if which == "66x12":
        p, n = grid(66, 12), 1
        cells, box = serpentine_cells(66, 0, 12)
        assert len(cells) == SERPENTINE_66 == 389 and box == (1, 0, 64, 10)
    elif which == "4k":
        p, n = grid(240, 135, margin=6), 8
        cells, box = serpentine_cells(240, 6, 129)
        assert len(cells) == 62 * 238 + 61 == 14817 and box == (1, 6, 238, 128)
    else:
        p, n = grid(120, 68, margin=3), 1
        cells = spiral_cells(1, 3, 118, 64)
        box = (1, 3, 118, 64)
        assert len(cells) > 3000 and len(set(cells)) == len(cells)
    mv, off, sd = batch_of([cells_frame(cells)] * n, len(cells))
    return Case(p, mv, off, sd, None, None, hand_of([(len(cells), 1, len(cells), box)] * n))


# ------------------------------------------------------------------ 5. many blobs

def domino_cells(gw, y_lo, y_hi):
    """Dominoes (x, y), (x + 1, y) with one free cell between them on every second analysed row, every other such row
    shifted by one column (a brick pattern): no two dominoes touch, each is a blob of two centres."""
    cells = []
    for i, y in enumerate(range(y_lo, y_hi, 2)):
        for x in range(1 + (i % 2), gw - 2, 3):
            cells += [(x, y), (x + 1, y)]
    return cells


@functools.lru_cache(maxsize=None)
def domino_case(which):
    """"1080p": 120 x 68, margin 3; "4k": 240 x 135, margin 6.  blobs = the number of dominoes (beyond any table of a
    bounded size), largest 2, the box that of the first one.  The expected values come from the model; these are what
    the construction says."""
    p = grid(120, 68, margin=3) if which == "1080p" else grid(240, 135, margin=6)
    mg = p.vertical_margin
    cells = domino_cells(p.grid_w, mg, p.grid_h - mg)
    mv, off, sd = batch_of([cells_frame(cells)], 5)
    n = len(cells) // 2
    return Case(p, mv, off, sd, None, None, hand_of([(2 * n, n, 2, (1, mg, 2, mg))]))


# ------------------------------------------------------------------ 6. one blob of everything

@functools.lru_cache(maxsize=None)
def everything_case(margin):
    """240 x 135, VECTORS_NEEDED 0, one frame with side data and no record, no mask: every cell of the grid is active,
    every analysed cell of columns 1 .. 238 is a centre, all of them one blob.  margin 6: 238 * 123 = 29 274, box (1, 6)
    .. (238, 128); margin 0: 238 * 135 = 32 130, box (1, 0) .. (238, 134)."""
    p = grid(240, 135, margin=margin, vn=0)
    rows = 135 - 2 * margin
    n = 238 * rows
    assert margin != 6 or n == 29274
    off, sd = frozen(np.zeros(2, dtype=np.uint64), np.ones(1, dtype=np.uint8))
    return Case(p, np.zeros(0, dtype=m.MV_DTYPE), off, sd, None, None, hand_of([(n, 1, n, (1, margin, 238, 134 - margin))]))


# ------------------------------------------------------------------ 7. tie and box

TIE_A = [(10, 2), (11, 2), (10, 3)]            # first cell (10, 2): index 2 * 20 + 10 = 50
TIE_B = [(3, 6), (4, 6), (5, 6)]               # first cell (3, 6): index 126 — further left, but later in row-major order


@functools.lru_cache(maxsize=None)
def tie_case():
    """20 x 12, margin 0.  Frame 0: blobs A and B of three cells each; A holds the smaller y * gw + x, so the box is A's,
    (10, 2) .. (11, 3), although B lies further left.  Frame 1: B grown by (6, 6): four cells, the box moves to (3, 6) ..
    (6, 6).  Frame 2: A grown by (11, 3) instead: the box is A's again."""
    p = grid(20, 12)
    mv, off, sd = batch_of([cells_frame(TIE_A + TIE_B), cells_frame(TIE_A + TIE_B + [(6, 6)]), cells_frame(TIE_A + [(11, 3)] + TIE_B)], 7)
    return Case(p, mv, off, sd, None, None, hand_of([(6, 2, 3, (10, 2, 11, 3)), (7, 2, 4, (3, 6, 6, 6)), (7, 2, 4, (10, 2, 11, 3))]))


# ------------------------------------------------------------------ 8. batch plumbing

@functools.lru_cache(maxsize=None)
def plumbing_case():
    """20 x 12, margin 0, nine frames:
        0 comb   1 U   2 ring, has_sd == 0 although it owns records   3 no side data, no record   4 tie frame 0
        5 comb   6 U   7 ring   8 comb
    streams (soff 0, 2, 2, 5, 6, 7): 0 = frames 0, 1, full mask; 1 empty; 2 = frames 2 .. 4, column 10 cleared; 3 = frame 5,
    all-zero mask; 4 = frame 6, full mask; frames 7 and 8 lie behind the last stream.
    Without a mask every frame with side data reads its shape's values.  With the masks:
        frame 4  column 10 cleared: A loses (10, 2) and (10, 3), (11, 2) is alone; B stays: 3 centres, 1 blob, box B's
        frame 5  nothing kept: 0;   frames 7, 8: behind the last stream: 0"""
    p = grid(20, 12)
    comb, u, ring, tie = cells_frame(comb_cells()), cells_frame(u_cells()), cells_frame(ring_cells()), cells_frame(TIE_A + TIE_B)
    mv, off, _ = batch_of([comb, u, ring, None, tie, comb, u, ring, comb], 8)
    sd = np.array([1, 1, 0, 0, 1, 1, 1, 1, 1], dtype=np.uint8)
    keeps = np.ones((5, 12, 20), dtype=bool)
    keeps[2, :, 10] = False
    keeps[3] = False
    soff = np.array([0, 2, 2, 5, 6, 7], dtype=np.uint64)
    none = (0, 0, 0, NO_BOX)
    c, uu, r, t = (95, 1, 95, (2, 1, 16, 11)), (24, 1, 24, (3, 2, 12, 9)), (35, 2, 32, (4, 2, 13, 9)), (6, 2, 3, (10, 2, 11, 3))
    plain = hand_of([c, uu, none, none, t, c, uu, r, c])
    masked = hand_of([c, uu, none, none, (3, 1, 3, (3, 6, 5, 6)), none, uu, none, none])
    return Case(p, mv, off, *frozen(sd, soff, keeps), {"plain": plain, "masked": masked})


# ------------------------------------------------------------------ 10. sweep equivalence

SWEEP_LEVELS = (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def sweep_case():
    """(params 1080p CLUSTERS_NEEDED 1 VECTORS_NEEDED 1, mv, off, sd, pts, soff): two streams of 48 frames at 25 fps.
    Frame f of a stream holds (f // 6) % 4 -> one run of 1, 2, 4 or 9 cells on row 30 (a run of 1 has no neighbour: no
    centre), and in every frame four separate pairs elsewhere — 8 centres that CLUSTERS_NEEDED 8 accepts and
    MIN_BLOB_CELLS 8 does not.  Stream 1 is stream 0 shifted by 12 frames."""
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1, clusters_needed=1)
    pairs = [(20, 10), (21, 10), (50, 12), (51, 12), (80, 14), (81, 14), (100, 40), (100, 41)]
    frames = []
    for s in range(2):
        for f in range(48):
            run = (1, 2, 4, 9)[((f + 12 * s) // 6) % 4]
            frames.append(cells_frame(pairs + [(40 + i, 30) for i in range(run)]))
    mv, off, sd = batch_of(frames, 10)
    pts = np.tile(np.arange(48, dtype=np.float64) / 25.0, 2)
    return (p, mv, off, sd) + frozen(pts, np.array([0, 48, 96], dtype=np.uint64))


# ------------------------------------------------------------------ 11. the LDS limit

def lds_by_hand(gw, R):
    """csrc/blobs_kernels.h: the tile ((R + 2) x gw 32-bit words padded to 16 bytes), R keep rows (the centre plane later),
    one plane of R + 2 mask rows, 32 bytes of totals."""
    W = (gw + 63) // 64
    return 4 * (((R + 2) * gw + 3) & ~3) + (2 * R + 2) * W * 8 + 32


def blobs_preview_or_none(p, lds=MI355X_LDS):
    try:
        return m.blobs_preview(p, lds)
    except m.MtgpuError as e:
        if e.code != m._abi.MT_ERR_UNSUPPORTED:
            raise
        return None


def _largest(ok, hi):
    assert ok(1)
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


LIMIT_TALL_GW, LIMIT_WIDE_GH = 65, 3


def limit_params(gw, gh, **kw):
    """Two-pixel cells keep every pixel coordinate of these grids inside int16."""
    p = m.ScanParams.from_config(2 * gw, 2 * gh, block_size=2, block_shift=1, vertical_mask=0.0, **kw)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (gw, gh, 0, 1)
    return p


@functools.lru_cache(maxsize=None)
def limit_shapes():
    """{"tall": (65, gh), "wide": (gw, 3)}: the last grids mtgpu_blobs_preview accepts at 163 840 bytes, found by
    bisection over the preview; one more row / column is MT_ERR_UNSUPPORTED."""
    tall = _largest(lambda gh: blobs_preview_or_none(limit_params(LIMIT_TALL_GW, gh)) is not None, 16383)

    def wide_ok(gw):
        p = limit_params(gw, LIMIT_WIDE_GH)
        try:
            m.plan_preview(p)
        except m.MtgpuError:
            return False
        return blobs_preview_or_none(p) is not None
    return {"tall": (LIMIT_TALL_GW, tall), "wide": (_largest(wide_ok, 16383), LIMIT_WIDE_GH)}


@functools.lru_cache(maxsize=None)
def limit_case(kind):
    """A serpentine over the whole grid, a frame of 30 random blobs (zones_inputs.clustered_frame) and a frame of pairs
    across the first and the last word seam on the first and the last row.  VECTORS_NEEDED 2 (the random blobs' cells
    hold 1 .. 4 votes); the shapes' cells get two votes.  Expected values: the model."""
    gw, gh = limit_shapes()[kind]
    p = limit_params(gw, gh, vectors_needed=2, clusters_needed=1, mv_threshold_sq=4.0)
    two = lambda cells: voters([(x, y, 2, 5, 0) for x, y in cells], 1)      # noqa: E731
    rng = np.random.RandomState(gw + gh)
    last = ((gw - 2) // 64) * 64
    seams = [(x, y) for y in (0, gh - 1) for s in {64, last} if 2 <= s <= gw - 2 for x in (s - 1, s)]
    mv, off, sd = batch_of([two(serpentine_cells(gw, 0, gh)[0]), zi.clustered_frame(rng, p, 30), two(seams)], 11)
    return Case(p, mv, off, sd, None, None, None)
