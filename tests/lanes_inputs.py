"""Inputs of tests/test_gpu_lanes.py (direction planes, include/mtgpu_lanes.h) with the values derived BY HAND from their
construction.  tests/test_lanes_host.py checks all of it against tests/lanes_model.py and, through the record filter of
consequence C, against the unchanged oracle, without a GPU.  Everything is built once per process and handed out
read-only.  A case is a dict: params, mv, off, sd, planes and soff — uint8 [S, gh, gw] with S + 1 frame offsets, or
uint8 [gh, gw] with soff None: one plane for every frame; hand_centres / hand_rose where the construction gives them.
The record builders, the streams and the random draws are those of tests/dir_inputs.py."""
import functools

import numpy as np

import mvtrim_amd as m

import dir_inputs as di
from derived_edge_inputs import frozen, voters

E, SE, S, SW, W, NW, N, NE = (1 << k for k in range(8))
ALL = 0xFF


def _case(p, frames, planes, soff=None, sd=None, **kw):
    c = dict(di._case(p, frames, sd=sd))
    for k in ("allow", "allows"):
        c.pop(k)
    c["planes"] = np.ascontiguousarray(planes, dtype=np.uint8)
    c["soff"] = None if soff is None else np.asarray(soff, dtype=np.uint64)
    assert c["planes"].shape == ((p.grid_h, p.grid_w) if soff is None else (len(soff) - 1, p.grid_h, p.grid_w))
    for k, v in kw.items():
        c[k] = np.asarray(v) if isinstance(v, (list, tuple)) else v
    frozen(*[v for v in c.values() if isinstance(v, np.ndarray) and v.flags.writeable])
    return c


def filled(p, byte, cells=()):
    """A plane of `byte` with single cells set: cells = [(x, y, byte)]."""
    plane = np.full((p.grid_h, p.grid_w), byte, dtype=np.uint8)
    for x, y, b in cells:
        plane[y, x] = b
    return plane


# ------------------------------------------------------------------ 1. frames derived by hand, on the 6 x 5 grid

@functools.lru_cache(maxsize=None)
def one_cell_case():
    """Two records of different sectors in ONE cell.  vectors_needed 2: cell (2, 1) holds an E and a W record, (3, 1) two
    E records.  Plane 0 lets E and W vote in (2, 1): two votes, both cells active, 2 centres.  Plane 1 lets only E vote
    there: one vote, inactive, (3, 1) is alone: 0.  Plane 2 lets only W vote in (2, 1) and nothing in (3, 1): 0.  The rose
    is 3 E and 1 W whatever the plane."""
    p = m.ScanParams.from_config(96, 80, **dict(di.SMALL_KW, vectors_needed=2))
    one = voters([(2, 1, 1, 5, 0), (2, 1, 1, -5, 0), (3, 1, 2, 5, 0)])
    planes = [filled(p, ALL, [(2, 1, E | W)]), filled(p, ALL, [(2, 1, E)]), filled(p, ALL, [(2, 1, W), (3, 1, 0)])]
    return _case(p, [one] * 3, planes, soff=[0, 1, 2, 3], hand_centres=[2, 0, 0], hand_rose=[[3, 0, 0, 0, 1, 0, 0, 0]] * 3)


@functools.lru_cache(maxsize=None)
def neighbours_case():
    """Two records of ONE sector in neighbouring cells whose bytes differ: (1, 3) and (2, 3) both move east.  Plane 0:
    E in (1, 3), W in (2, 3): one active cell, 0 centres.  Plane 1: E in both: 2.  Plane 2: everything but E in both: 0."""
    p = m.ScanParams.from_config(96, 80, **di.SMALL_KW)
    one = voters([(1, 3, 1, 5, 0), (2, 3, 1, 5, 0)])
    planes = [filled(p, 0, [(1, 3, E), (2, 3, W)]), filled(p, 0, [(1, 3, E), (2, 3, E)]), filled(p, ALL, [(1, 3, ALL & ~E), (2, 3, ALL & ~E)])]
    return _case(p, [one] * 3, planes, soff=[0, 1, 2, 3], hand_centres=[0, 2, 0], hand_rose=[[2, 0, 0, 0, 0, 0, 0, 0]] * 3)


@functools.lru_cache(maxsize=None)
def still_case():
    """Threshold 0 and a plane of zeros: the still records in (1, 1) and (2, 1) vote (no direction to object to) and are in
    no bin, the record that moves east in (3, 1) counts in the rose and does not vote: 2 centres.  With E in (3, 1): 3."""
    p = m.ScanParams.from_config(96, 80, **dict(di.SMALL_KW, mv_threshold_sq=0.0))
    one = voters([(1, 1, 1, 0, 0), (2, 1, 1, 0, 0), (3, 1, 1, 5, 0)])
    return _case(p, [one, one], [filled(p, 0), filled(p, 0, [(3, 1, E)])], soff=[0, 1, 2], hand_centres=[2, 3],
                 hand_rose=[[1, 0, 0, 0, 0, 0, 0, 0]] * 2)


@functools.lru_cache(maxsize=None)
def vn0_case():
    """vectors_needed == 0 (consequence F): every cell of the grid is active whatever the plane holds: 5 rows x columns
    1 .. 4 = 20; a frame with side data and no record: the same, an empty rose."""
    p = m.ScanParams.from_config(96, 80, **dict(di.SMALL_KW, vectors_needed=0))
    one = voters(di.BOUNDARY_CELLS)
    planes = [filled(p, 0), filled(p, ALL), filled(p, W)]
    return _case(p, [one, one, one[:0]], planes, soff=[0, 1, 2, 3], hand_centres=[20, 20, 20],
                 hand_rose=[di.BOUNDARY_ROSE, di.BOUNDARY_ROSE, [0] * 8])


@functools.lru_cache(maxsize=None)
def margin_case():
    """6 x 8 cells, margin 1 (analysed rows 1 .. 6), every record moves east, the plane's margin rows hold 0 and the rest
    everything.  (2, 0) and (4, 7) lie in the margin rows: they do not count — no bin, no vote, their bytes are not
    looked at — so (2, 1) and (4, 6) next to them have no active neighbour; the pair (1, 3) + (2, 3) gives 2 centres.
    rose[E] = 4.  Plane 1 holds 0xFF in the margin rows: the same values."""
    p = m.ScanParams.from_config(96, 128, **dict(di.SMALL_KW, vertical_mask=0.125))
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (6, 8, 1)
    one = voters([(2, 0, 1, 5, 0), (2, 1, 1, 5, 0), (4, 7, 1, 5, 0), (4, 6, 1, 5, 0), (1, 3, 1, 5, 0), (2, 3, 1, 5, 0)])
    zero_margin = filled(p, ALL)
    zero_margin[0], zero_margin[7] = 0, 0
    return _case(p, [one, one], [zero_margin, filled(p, ALL)], soff=[0, 1, 2], hand_centres=[2, 2],
                 hand_rose=[[4, 0, 0, 0, 0, 0, 0, 0]] * 2)


HAND_CASES = {"one_cell": one_cell_case, "neighbours": neighbours_case, "still": still_case, "vn0": vn0_case, "margin": margin_case}


# ------------------------------------------------------------------ 2. word seams, by hand

# The records of dir_inputs.SEAM_64 / SEAM_128 (rows 1, 3, 5, 7 of a nine-row grid, E and W around columns 63 | 64 and
# 127 | 128).  The plane's bytes change exactly there: columns 0 .. 63, 64 .. 127 and 128 hold a, b, a.  Stream 0 has
# (a, b) = (E, W), stream 1 (W, E); a plane is 9 gw bytes, an odd number, so plane 1 begins on an odd byte address.
#   65 wide (64 is the last column: a neighbour, never a centre)
#     stream 0   row 1: 63 alone; row 3: 63 E and 64 W both vote: 63 is a centre; row 5: none; row 7: 63 alone      = 1
#     stream 1   row 1: 64 alone; row 3: none; row 5: 63 W and 64 E: 63; row 7: 62 and 64, apart                     = 1
#   129 wide (64 can be a centre now; 128 is the last column)
#     stream 0   row 1: 63, 126, 128, apart; row 3: 63, 64: both centres; 127, 128 do not vote; rows 5, 7 as above   = 2
#     stream 1   row 1: 64, 127, apart; row 3: 127 E and 128 W vote: 127; row 5: 63, 64: 2; row 7: 62, 64, apart     = 3
SEAM_HAND = {65: [1, 1], 129: [2, 3]}


def seam_planes(p):
    x = np.arange(p.grid_w)
    first = np.where((x >= 64) & (x < 128), W, E).astype(np.uint8)
    second = np.where((x >= 64) & (x < 128), E, W).astype(np.uint8)
    return np.stack([np.tile(first, (p.grid_h, 1)), np.tile(second, (p.grid_h, 1))])


@functools.lru_cache(maxsize=None)
def seam_case(gw):
    d = di.seam_case(gw)
    p = d["params"]
    cells = di.SEAM_64 + (di.SEAM_128 if gw == 129 else [])
    one = voters([(x, y, 1) + di.DISP[s] for x, y, s in cells])
    rose = np.bincount([s for _, _, s in cells], minlength=8)
    assert (p.grid_w * p.grid_h) % 2 == 1
    return _case(p, [one] * 2, seam_planes(p), soff=[0, 1, 2], hand_centres=SEAM_HAND[gw], hand_rose=[rose] * 2)


# ------------------------------------------------------------------ 3. the two forms on the 4K grid

def cellwise_plane(p):
    """Bytes that differ cell by cell: (x * 7 + y * 13) & 0xFF."""
    y, x = np.mgrid[0:p.grid_h, 0:p.grid_w]
    return ((x * 7 + y * 13) & 0xFF).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def uhd_case(vertical_mask):
    """3840 x 2160: 240 x 135 cells.  vertical_mask 0: the plane's 135 rows do not fit next to the tile (the unstaged
    form); 0.05: margin 6, the staged form.  Four frames of a few hundred records in blobs all over the grid, every
    record with a direction of its own; one plane for every frame."""
    p = m.ScanParams.from_config(3840, 2160, mv_threshold_sq=4.0, block_size=16, block_shift=4, vectors_needed=2, clusters_needed=1,
                                 vertical_mask=vertical_mask)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (240, 135, 6 if vertical_mask else 0)
    rng = np.random.RandomState(2160)
    frames = [di.directed_frame(rng, p, 40 + 10 * f) for f in range(4)]
    return _case(p, frames, cellwise_plane(p))


# ------------------------------------------------------------------ 4. a frame in three pieces

PIECES_N, PIECES_COLUMN, PIECES_SECTOR = 300000, 5, 3


@functools.lru_cache(maxsize=None)
def pieces_case():
    """Two frames of 300 000 records each — three pieces of the kernel's 131 072 — that all move south-west into column 5
    of the 80 x 6 grid, row i % 6.  Plane 0 forbids SW in rows 0 .. 2, half of the column's cells: rows 3, 4, 5 hold
    50 000 votes each and a neighbour: 3 centres.  Plane 1 allows everything: 6.  rose[SW] = 300 000 for both."""
    p = m.ScanParams.from_config(1280, 96, **dict(di.SMALL_KW, vectors_needed=3))
    assert (p.grid_w, p.grid_h) == (80, 6)
    i = np.arange(PIECES_N, dtype=np.int64)
    d = di.DISP[PIECES_SECTOR]
    mv = np.zeros(PIECES_N, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = PIECES_COLUMN * 16 + 8, (i % 6) * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - d[0], mv["dst_y"] - d[1]
    half = filled(p, ALL)
    half[0:3, :] = ALL & ~(1 << PIECES_SECTOR)
    rose = [0] * 8
    rose[PIECES_SECTOR] = PIECES_N
    return _case(p, [mv, mv], [half, filled(p, ALL)], soff=[0, 1, 2], hand_centres=[3, 6], hand_rose=[rose, rose])


# ------------------------------------------------------------------ 5. streams

@functools.lru_cache(maxsize=None)
def stream_case():
    """dir_inputs.stream_case's batch — seven streams of 0, 1, 2, 64, 0, 0 and 33 frames, three frames in front and five
    behind that hold records and belong to no stream, a key frame inside the fourth — with seven different planes."""
    d = di.stream_case()
    p = d["params"]
    rng = np.random.RandomState(707)
    planes = rng.randint(0, 256, size=(len(di.STREAM_SIZES), p.grid_h, p.grid_w)).astype(np.uint8)
    planes[3] |= E | W                              # the long stream keeps most of its centres
    c = dict(d, planes=planes)
    for k in ("allow", "allows", "scalar_allow"):
        c.pop(k)
    frozen(planes)
    return c


# ------------------------------------------------------------------ 6. random draws for the consequences

N_DRAWS = di.N_DRAWS
N_FLOW_DRAWS = 20


@functools.lru_cache(maxsize=None)
def draw(i):
    """dir_inputs.draw(i) — grid, vectors_needed, margin and records — with a chain of planes, each a subset of the next
    in every cell (consequence D): zeros, a & b, a, a | c, 0xFF for random a, b, c; `zones`: a plane whose bytes are 0x00
    or 0xFF (consequence E); `planes`: a, one plane for every frame."""
    d = di.draw(i)
    p = d["params"]
    rng = np.random.RandomState(9000 + i)
    a, b, c = (rng.randint(0, 256, size=(p.grid_h, p.grid_w)).astype(np.uint8) for _ in range(3))
    chain = [np.zeros_like(a), a & b, a, a | c, np.full_like(a, ALL)]
    zones = np.where(rng.rand(p.grid_h, p.grid_w) < 0.7, ALL, 0).astype(np.uint8)
    out = dict(params=p, mv=d["mv"], off=d["off"], sd=d["sd"], chain=chain, zones=zones, planes=a, soff=None)
    frozen(*chain, zones)
    return out
