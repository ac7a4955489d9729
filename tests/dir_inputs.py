"""Inputs of tests/test_gpu_dir.py (the direction filter, include/mtgpu_dir.h) with the values derived BY HAND from their
construction.  tests/test_dir_host.py checks all of it against tests/dir_model.py and, through the record filter of
consequence C, against the unchanged oracle, without a GPU.  Everything is built once per process and handed out
read-only.  A case is a dict: params, mv, off, sd, and soff / allows (one allow byte per stream) or allow (one byte for
every frame); hand_centres / hand_rose where the construction gives them."""
import dataclasses
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import direction, synth

from derived_edge_inputs import BIG_KW, frozen, voters
from derived_soak import SHIFT_P
from scan_checks import junk_padding

# one displacement per sector, |d|^2 = 25 or 32
DISP = [(5, 0), (4, 4), (0, 5), (-4, 4), (-5, 0), (-4, -4), (0, -5), (4, -4)]
# the boundary table of include/mtgpu_dir.h
BOUNDARY = [((12, 5), 0), ((12, 6), 1), ((5, 12), 2), ((3, 1), 0), ((2, 1), 1), ((65535, 27306), 0), ((65535, 27307), 1)]
SMALL_KW = dict(mv_threshold_sq=4.0, block_size=16, block_shift=4, vectors_needed=1, clusters_needed=1, vertical_mask=0.0)


def _case(p, frames, sd=None, **kw):
    b = m.FrameBatch.from_frames(frames)
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, np.random.RandomState(len(mv)))
    sd = np.ones(len(frames), dtype=np.uint8) if sd is None else np.asarray(sd, dtype=np.uint8)
    out = dict(params=p, mv=mv, off=np.ascontiguousarray(b.frame_off, dtype=np.uint64), sd=sd, soff=None, allows=None, allow=0xFF)
    for k, v in kw.items():
        out[k] = np.asarray(v) if isinstance(v, (list, tuple)) else v
    if out["soff"] is not None:
        out["soff"] = np.asarray(out["soff"], dtype=np.uint64)
        out["allows"] = np.asarray(out["allows"], dtype=np.uint8)
    frozen(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


# ------------------------------------------------------------------ 1. frames derived by hand

# The five boundary points with small displacements, one record each, on the 6 x 5 grid (margin 0, one vote makes a cell
# active):  row 1: (1, 1) <- (12, 5) E, (2, 1) <- (12, 6) SE, (3, 1) <- (5, 12) S;  row 3: (1, 3) <- (3, 1) E,
# (2, 3) <- (2, 1) SE.  Columns 1 .. 4 can be centres.
#   allow      active cells                                  centres
#   all        row 1: 1, 2, 3; row 3: 1, 2                   3 + 2 = 5
#   E          (1, 1), (1, 3): no neighbours                 0
#   E|SE       row 1: 1, 2; row 3: 1, 2                      2 + 2 = 4
#   S          (3, 1) alone                                  0
#   SE|S       row 1: 2, 3; row 3: 2 alone                   2
#   none       nothing                                       0
# The rose is [2, 2, 1, 0, 0, 0, 0, 0] under every allow.
BOUNDARY_CELLS = [(1, 1, 1, 12, 5), (2, 1, 1, 12, 6), (3, 1, 1, 5, 12), (1, 3, 1, 3, 1), (2, 3, 1, 2, 1)]
BOUNDARY_ALLOWS = [0xFF, 0x01, 0x03, 0x04, 0x06, 0x00]
BOUNDARY_HAND = [5, 0, 4, 0, 2, 0]
BOUNDARY_ROSE = [2, 2, 1, 0, 0, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def boundary_case():
    """Six streams of one frame, the same five records, one allow byte each."""
    p = m.ScanParams.from_config(96, 80, **SMALL_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (6, 5, 0)
    n = len(BOUNDARY_ALLOWS)
    return _case(p, [voters(BOUNDARY_CELLS)] * n, soff=np.arange(n + 1), allows=BOUNDARY_ALLOWS, hand_centres=BOUNDARY_HAND,
                 hand_rose=[BOUNDARY_ROSE] * n)


@functools.lru_cache(maxsize=None)
def zero_case():
    """Threshold 0: two still records in (1, 1) and (2, 1) and one that moves east in (3, 1).  allow = 0: the still ones
    vote (no direction to object to) and are in no bin: 2 centres, rose[E] = 1.  allow = E: 3 centres, the same rose."""
    p = m.ScanParams.from_config(96, 80, **dict(SMALL_KW, mv_threshold_sq=0.0))
    one = voters([(1, 1, 1, 0, 0), (2, 1, 1, 0, 0), (3, 1, 1, 5, 0)])
    return _case(p, [one, one], soff=[0, 1, 2], allows=[0x00, 0x01], hand_centres=[2, 3], hand_rose=[[1, 0, 0, 0, 0, 0, 0, 0]] * 2)


@functools.lru_cache(maxsize=None)
def vn0_case():
    """vectors_needed == 0 (consequence F): every cell of the grid is active, whatever votes: 5 rows x columns 1 .. 4 = 20
    under allow = 0 and under all; a frame with side data and no record: the same, an empty rose."""
    p = m.ScanParams.from_config(96, 80, **dict(SMALL_KW, vectors_needed=0))
    one = voters(BOUNDARY_CELLS)
    return _case(p, [one, one, one[:0]], soff=[0, 1, 2, 3], allows=[0x00, 0xFF, 0x10], hand_centres=[20, 20, 20],
                 hand_rose=[BOUNDARY_ROSE, BOUNDARY_ROSE, [0] * 8])


@functools.lru_cache(maxsize=None)
def margin_case():
    """6 x 8 cells, margin 1 (analysed rows 1 .. 6), every record moves east.  (2, 0) and (4, 7) lie in the margin rows:
    they do not count — no bin, no vote — so (2, 1) and (4, 6) right next to them have no active neighbour; the pair
    (1, 3) + (2, 3) gives 2 centres.  rose[E] = 4."""
    p = m.ScanParams.from_config(96, 128, **dict(SMALL_KW, vertical_mask=0.125))
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (6, 8, 1)
    one = voters([(2, 0, 1, 5, 0), (2, 1, 1, 5, 0), (4, 7, 1, 5, 0), (4, 6, 1, 5, 0), (1, 3, 1, 5, 0), (2, 3, 1, 5, 0)])
    return _case(p, [one, one], soff=[0, 1, 2], allows=[0xFF, 0x01], hand_centres=[2, 2], hand_rose=[[4, 0, 0, 0, 0, 0, 0, 0]] * 2)


HAND_CASES = {"boundary": boundary_case, "zero": zero_case, "vn0": vn0_case, "margin": margin_case}


# ------------------------------------------------------------------ 2. the streamers' edges

EDGE_LENGTHS = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 8207]
EDGE_ALLOW = 0xA5                                      # E, S, NW, NE


def edge_frame(n):
    """n records on the 80 x 6 grid: record i lies in cell c = (i * i // 7 + i // 3) % 480, column c % 80 of row c // 80 —
    an uneven spread, so that under vectors_needed 6 some cells are active and some are not, with and without the mask —
    and moves towards sector (i + i // 8) % 8: never the sector of the record before or behind it."""
    i = np.arange(n, dtype=np.int64)
    sec = (i + i // 8) % 8
    d = np.array(DISP, dtype=np.int64)[sec]
    cell = (i * i // 7 + i // 3) % 480
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = (cell % 80) * 16 + 8, (cell // 80) * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - d[:, 0], mv["dst_y"] - d[:, 1]
    return mv


def edge_rose(n):
    i = np.arange(n, dtype=np.int64)
    return np.bincount((i + i // 8) % 8, minlength=8)


@functools.lru_cache(maxsize=None)
def edge_case():
    """For each of the sixteen 8-byte phases of a 128-byte line, one frame of each length of EDGE_LENGTHS whose first
    record starts on that phase when the record array starts on a line — record index = phase (mod 16) for compact
    records, 5 x index = phase (mod 16) for 40-byte ones, so over the sixteen residues both sizes meet every phase.  In
    front of each test frame a frame WITHOUT side data holds the 0 .. 15 records that move the start there; they move east
    into (1, 1) and (2, 1), so a read outside a frame shows in its rose.  test: the test frames' indices; start: the
    record index each starts on."""
    p = m.ScanParams.from_config(1280, 96, **dict(SMALL_KW, vectors_needed=6))
    assert (p.grid_w, p.grid_h) == (80, 6)
    frames, sd, test, start, at = [], [], [], [], 0
    for phase in range(16):
        for n in EDGE_LENGTHS:
            pad = (phase - at) % 16
            frames.append(voters([(1 + j % 2, 1, 1, 5, 0) for j in range(pad)]))
            sd.append(0)
            at += pad
            test.append(len(frames))
            start.append(at)
            frames.append(edge_frame(n))
            sd.append(1)
            at += n
    assert all(s % 16 == i // len(EDGE_LENGTHS) for i, s in enumerate(start))
    F = len(frames)
    hand_rose = np.zeros((F, 8), dtype=np.int64)
    for f, n in zip(test, EDGE_LENGTHS * 16):
        hand_rose[f] = edge_rose(n)
    return _case(p, frames, sd=sd, allow=EDGE_ALLOW, test=np.array(test), start=np.array(start), hand_rose=hand_rose)


# ------------------------------------------------------------------ 3. word seams, by hand

# Rows 1, 3, 5, 7 of a nine-row grid, E and W records around columns 63 | 64 (two rows apart: no vertical neighbours):
#   row 1: 63 E, 64 E          row 3: 63 E, 64 W          row 5: 63 W, 64 E          row 7: 62 W, 63 E, 64 E
# On the 65-wide grid 64 is the last column: a neighbour, never a centre.
#   all   row 1: 63; row 3: 63; row 5: 63; row 7: 62, 63                                                 =  5
#   E     row 1: 63, its neighbour 64 across the seam is active; rows 3, 5: one cell alone; row 7: 63    =  2
#   W     at most one cell per row                                                                       =  0
# On the 129-wide grid both columns can be centres, and the seam 127 | 128 is added, where 128 is the last column:
#   row 1: 126 W, 127 E, 128 E                row 3: 127 E, 128 W
#   all   2 + 2 + 2 + 3 = 9, + 2 (126, 127) + 1 (127)                                                    = 12
#   E     row 1: 2; rows 3, 5: 0; row 7: 63, 64: 2; + 1 (127, its neighbour 128 is active) + 0           =  5
#   W     0
SEAM_64 = [(63, 1, 0), (64, 1, 0), (63, 3, 0), (64, 3, 4), (63, 5, 4), (64, 5, 0), (62, 7, 4), (63, 7, 0), (64, 7, 0)]
SEAM_128 = [(126, 1, 4), (127, 1, 0), (128, 1, 0), (127, 3, 0), (128, 3, 4)]
SEAM_ALLOWS = [0xFF, 0x01, 0x10]
SEAM_HAND = {65: [5, 2, 0], 129: [12, 5, 0]}


@functools.lru_cache(maxsize=None)
def seam_case(gw):
    p = m.ScanParams.from_config(gw * 16, 144, **SMALL_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (gw, 9, 0)
    cells = SEAM_64 + (SEAM_128 if gw == 129 else [])
    one = voters([(x, y, 1) + DISP[s] for x, y, s in cells])
    rose = np.bincount([s for _, _, s in cells], minlength=8)
    return _case(p, [one] * 3, soff=[0, 1, 2, 3], allows=SEAM_ALLOWS, hand_centres=SEAM_HAND[gw], hand_rose=[rose] * 3)


# ------------------------------------------------------------------ 4. the width of the rose's counters

WIDTH_N, WIDTH_SECTOR = 300000, 3


@functools.lru_cache(maxsize=None)
def width_case():
    """One frame of 300 000 records that move south-west — more than 256 x 1024 — and one record of each other sector, spread
    through the frame.  rose = 300 000 in sector 3, 1 in each of the others."""
    p = m.ScanParams.from_config(1280, 96, **dict(SMALL_KW, vectors_needed=3))
    n = WIDTH_N + 7
    i = np.arange(n, dtype=np.int64)
    sec = np.full(n, WIDTH_SECTOR, dtype=np.int64)
    others = [s for s in range(8) if s != WIDTH_SECTOR]
    sec[[1 + 40000 * j for j in range(7)]] = others
    d = np.array(DISP, dtype=np.int64)[sec]
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = (i % 80) * 16 + 8, ((i // 80) % 6) * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - d[:, 0], mv["dst_y"] - d[:, 1]
    rose = np.ones(8, dtype=np.int64)
    rose[WIDTH_SECTOR] = WIDTH_N
    return _case(p, [mv], allow=0xFF & ~(1 << WIDTH_SECTOR), hand_rose=[rose])


# ------------------------------------------------------------------ 5. extreme displacements

# (dst_x, dst_y, src_x, src_y) on the 32 x 32 grid of 1024-pixel cells, and what becomes of the record:
EXTREME_RECORDS = [
    (32767, 100, -32768, 100),      # (65535, 0)        E, cell (31, 0)
    (-32768, 100, 32767, 100),      # (-65535, 0)       dst outside the grid: does not count
    (100, 32767, 100, -32768),      # (0, 65535)        S, cell (0, 31)
    (100, -32768, 100, 32767),      # (0, -65535)       dst outside the grid: does not count
    (32767, 27306, -32768, 0),      # (65535, 27306)    E: 12 x 27306 = 327672 <= 327675
    (32767, 27307, -32768, 0),      # (65535, 27307)    SE: 327684 > 327675
    (0, 5000, 32767, 5000),         # (-32767, 0)       W
    (5000, 0, 5000, 32767),         # (0, -32767)       N
    (0, 14652, 32767, 1000),        # (-32767, 13652)   W: 163824 <= 163835
    (0, 14653, 32767, 1000),        # (-32767, 13653)   SW: 163836 > 163835
]
EXTREME_ROSE = [2, 1, 1, 1, 2, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def extreme_case():
    p = m.ScanParams.from_config(32768, 32768, mv_threshold_sq=4.0, vectors_needed=1, clusters_needed=1, **BIG_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (32, 32, 0)
    mv = np.zeros(len(EXTREME_RECORDS), dtype=m.MV_DTYPE)
    a = np.array(EXTREME_RECORDS, dtype=np.int64)
    mv["dst_x"], mv["dst_y"], mv["src_x"], mv["src_y"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return _case(p, [mv, mv], soff=[0, 1, 2], allows=[0xFF, 0x11], hand_rose=[EXTREME_ROSE] * 2)


# ------------------------------------------------------------------ clustered frames with directions

def directed_frame(rng, p, n_blobs, sectors=None):
    """Blobs of 2 x 2 or 3 x 2 neighbouring cells with 1 .. 4 votes each; every record moves towards a sector of its own
    (drawn from `sectors`, default all eight) with DISP or, one in four, a boundary displacement; a still record and two
    outside the grid."""
    pool = list(range(8)) if sectors is None else list(sectors)
    cells = []
    for _ in range(n_blobs):
        x0, y0 = rng.randint(0, max(p.grid_w - 2, 1)), rng.randint(0, max(p.grid_h - 1, 1))
        for cx in range(2 + rng.randint(0, 2)):
            for cy in range(2):
                if x0 + cx < p.grid_w and y0 + cy < p.grid_h:
                    for _ in range(int(rng.randint(1, 5))):
                        s = int(rng.choice(pool))
                        d = DISP[s]
                        if rng.rand() < 0.25:
                            (bx, by), bs = BOUNDARY[int(rng.randint(0, 5))]
                            # the table's points lie in sectors 0 .. 2; turned by two sectors at a time they cover the rest
                            for _ in range((s - bs) // 2 % 4):
                                bx, by = -by, bx
                            d = (bx, by)
                        cells.append((x0 + cx, y0 + cy, 1, d[0], d[1]))
    cells += [(int(rng.randint(0, p.grid_w)), int(rng.randint(0, p.grid_h)), 1, 0, 0), (p.grid_w + 1, 1, 1, 5, 0),
              (2, p.grid_h + 2, 1, 0, 5)]
    mv = voters(cells, p.block_shift)
    return mv[rng.permutation(len(mv))]


# ------------------------------------------------------------------ 6. streams

STREAM_SIZES = [0, 1, 2, 64, 0, 0, 33]
STREAM_ALLOWS = [0xFF, 0x01, 0x10, 0x0F, 0xAA, 0x55, 0xF0]
STREAM_FRONT, STREAM_BEHIND = 3, 5
STREAM_KEY_FRAME = 3 + 1 + 2 + 20                       # inside the stream of 64 frames


@functools.lru_cache(maxsize=None)
def stream_case():
    """Seven streams of 0, 1, 2, 64, 0, 0 and 33 frames with an allow byte each; three frames in front of stream_off[0]
    and five behind stream_off[7] hold records like the others and belong to no stream; one frame inside the fourth
    stream is a key frame without side data (and holds records)."""
    p = m.ScanParams.from_config(1280, 96, **dict(SMALL_KW, vectors_needed=2, clusters_needed=2))
    rng = np.random.RandomState(606)
    F = STREAM_FRONT + sum(STREAM_SIZES) + STREAM_BEHIND
    frames = [directed_frame(rng, p, 6 + f % 4) for f in range(F)]
    sd = np.ones(F, dtype=np.uint8)
    sd[STREAM_KEY_FRAME] = 0
    soff = STREAM_FRONT + np.concatenate([[0], np.cumsum(STREAM_SIZES)])
    return _case(p, frames, sd=sd, soff=soff, allows=STREAM_ALLOWS, scalar_allow=0x0F)


# ------------------------------------------------------------------ 7. random draws for the consequences

N_DRAWS = 40
DRAW_ALLOWS = [0x00, 0x01, 0x11, 0x1B, 0x5B, 0xDB, 0xFF]          # a chain: each a subset of the next (consequence E)


def _turnable(mv):
    """Records whose src can be replaced by dst - (-dy, dx) and by dst - (-dx, dy) inside int16."""
    dx = mv["dst_x"].astype(np.int64) - mv["src_x"]
    dy = mv["dst_y"].astype(np.int64) - mv["src_y"]
    ok = np.ones(len(mv), dtype=bool)
    for sx, sy in ((mv["dst_x"] + dy, mv["dst_y"] - dx), (mv["dst_x"] + dx, mv["src_y"].astype(np.int64))):
        ok &= (sx >= -32768) & (sx <= 32767) & (sy >= -32768) & (sy <= 32767)
    return ok


def rotated(mv):
    """Every displacement (dx, dy) -> (-dy, dx): a quarter turn clockwise on the screen; dst stays."""
    out = mv.copy()
    dx = mv["dst_x"].astype(np.int64) - mv["src_x"]
    dy = mv["dst_y"].astype(np.int64) - mv["src_y"]
    out["src_x"], out["src_y"] = mv["dst_x"] + dy, mv["dst_y"] - dx
    return out


def mirrored(mv):
    """Every displacement (dx, dy) -> (-dx, dy); dst stays."""
    out = mv.copy()
    dx = mv["dst_x"].astype(np.int64) - mv["src_x"]
    out["src_x"] = mv["dst_x"] + dx
    return out


@functools.lru_cache(maxsize=None)
def draw(i):
    """Draw i of N_DRAWS: a grid of the soak's set (w in [64, 3900), h in [64, 2200), block_shift 1 .. 5 with the soak's
    weights) that the direction scan supports, vectors_needed i % 4, a margin of (i // 4) % 4 rows where the grid has
    more than twice as many, up to 12 frames of up to 2 700 random records plus at most 291 of blobs whose records move in
    every direction: up to 3 000; only records that can be turned and mirrored inside int16 are kept (consequence D)."""
    rng = np.random.RandomState(7000 + i)
    while True:
        sh = int(rng.choice([1, 2, 3, 4, 5], p=SHIFT_P))
        w, h = int(rng.randint(64, 3900)), int(rng.randint(64, 2200))
        p = m.ScanParams.from_config(w, h, mv_threshold_sq=float(rng.choice([16.0, 4.0, 0.0, 9.5])), block_size=1 << sh, block_shift=sh,
                                     vectors_needed=i % 4, clusters_needed=int(rng.choice([1, 2, 3])), vertical_mask=0.0)
        margin = (i // 4) % 4
        if 2 * margin >= p.grid_h:
            margin = 0
        p = dataclasses.replace(p, vertical_margin=margin)
        try:
            m.plan_preview(p)
            m.dir_preview(p)
            break
        except m.MtgpuError:
            continue
    F = int(rng.randint(1, 13))
    mv, off, _ = synth.random_frames(rng, F, 2700, w, h, hot=float(rng.choice([0.05, 0.5, 0.95])))
    frames = []
    for f in range(F):
        part = np.concatenate([mv[int(off[f]):int(off[f + 1])], directed_frame(rng, p, 4 + 4 * (f % 3))])
        part = part[_turnable(part)]
        frames.append(part[rng.permutation(len(part))])
    sd = (rng.rand(F) < 0.85).astype(np.uint8)
    sd[0] = 1
    return _case(p, frames, sd=sd)
