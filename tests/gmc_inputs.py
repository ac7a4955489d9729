"""Inputs of tests/test_gpu_gmc.py and tests/test_gmc_host.py (global-motion compensation, include/mtgpu_gmc.h) with the
values derived BY HAND from their construction.  The hand cases live on an 8 x 6 grid (128 x 96 pixels, 16-pixel cells,
VERTICAL_MASK 0) and on the same grid with a one-row margin (VERTICAL_MASK 0.2); vectors_needed 1, clusters_needed 1
unless a case says otherwise.  Every record comes from derived_edge_inputs.voters: cells = [(gx, gy, votes, dx, dy)],
dst in the middle of the cell, dst - src = (dx, dy).  Everything is built once per process and handed out read-only."""
import functools

import numpy as np

import mvtrim_amd as m

from derived_edge_inputs import frozen, voters

GW, GH = 8, 6


def hand_params(thr=16.0, margin=0, vn=1):
    p = m.ScanParams.from_config(128, 96, mv_threshold_sq=float(thr), block_size=16, block_shift=4, vectors_needed=vn,
                                 clusters_needed=1, vertical_mask=0.2 if margin else 0.0)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (GW, GH, margin)
    return p


def _pan(dx, dy, other=None):
    """One record per cell of the whole grid with (dx, dy); other: {(x, y): (dx, dy)} for the cells that differ."""
    other = other or {}
    return [(x, y, 1) + other.get((x, y), (dx, dy)) for y in range(GH) for x in range(GW)]


_SUPPORT = [(1, 1, 2, 5, 0), (2, 1, 2, 5, 0), (0, 3, 1, 7, 0), (7, 3, 1, 8, 0), (0, 5, 1, 9, 0), (7, 5, 1, 10, 0)]
_EDGE = [(1, 1, 2, 4, 0), (2, 1, 1, 4, 0), (5, 4, 2, 5, 0)]

# name -> (thr, margin, cells, max_shift, min_share_q8, (gx, gy, mode_x, mode_y, n_in, n_x, n_y), centres, plain centres)
# `plain centres`: the count of the uncompensated scan of the same frame, by hand as well.
HAND = {
    # every cell moves by (5, 0): the plain scan sees 6 x 6 centres (columns 1 .. 6, every row), the residuals are 0
    "pure_pan": (16, 0, _pan(5, 0), 16, 128, (5, 0, 5, 0, 48, 48, 48), 0, 36),
    "pure_pan_share_256": (16, 0, _pan(5, 0), 16, 256, (5, 0, 5, 0, 48, 48, 48), 0, 36),      # 48 * 256 >= 256 * 48
    "pan_diagonal": (16, 0, _pan(-3, 7), 16, 128, (-3, 7, -3, 7, 48, 48, 48), 0, 36),
    # a 2 x 2 object at dx 11 inside the pan: hx[5] = 44, hx[11] = 4; the object's residual is 6, 36 >= 16: 4 cells, each
    # with a neighbour
    "pan_plus_object": (16, 0, _pan(5, 0, {(x, y): (11, 0) for x in (3, 4) for y in (2, 3)}), 16, 128,
                        (5, 0, 5, 0, 48, 44, 48), 4, 36),
    # four records at -1, four at +1, one at 0: -1 comes first in the walk.  4 * 256 >= 64 * 9.  Threshold 4: the +1 cells
    # (2, 1) and (3, 1) have residual 2 and are neighbours: 2 (with +1 applied, (1, 1) alone would be kept: 0)
    "tie_minus_plus": (4, 0, [(1, 1, 4, -1, 0), (2, 1, 2, 1, 0), (3, 1, 2, 1, 0), (5, 4, 1, 0, 0)], 16, 64,
                       (-1, 0, -1, 0, 9, 4, 9), 2, 0),
    # three records at 0, three at 2: 0 comes first, and 3 * 256 == 128 * 6: support exactly met.  The cells at 2 keep
    # their residual 2, 4 >= 4: two neighbours
    "tie_zero_two": (4, 0, [(1, 1, 3, 0, 0), (4, 3, 2, 2, 0), (5, 3, 1, 2, 0)], 16, 128, (0, 0, 0, 0, 6, 3, 6), 2, 2),
    # four of eight records at 5: 4 * 256 == 128 * 8.  The four others (7, 8, 9, 10) sit alone in columns 0 and 7
    "support_met": (16, 0, _SUPPORT, 16, 128, (5, 0, 5, 0, 8, 4, 8), 0, 2),
    # one more record elsewhere: 4 * 256 < 128 * 9, nothing is applied on x
    "support_one_short": (16, 0, _SUPPORT + [(7, 0, 1, 6, 0)], 16, 128, (0, 0, 5, 0, 9, 4, 9), 2, 2),
    # one record at 5, one at 6: 5 comes first.  min_share 0 applies it, residuals 0 and 1; min_share 256 does not
    "share_zero": (16, 0, [(1, 1, 1, 5, 0), (2, 1, 1, 6, 0)], 16, 0, (5, 0, 5, 0, 2, 1, 2), 0, 2),
    "share_256_unmet": (16, 0, [(1, 1, 1, 5, 0), (2, 1, 1, 6, 0)], 16, 256, (0, 0, 5, 0, 2, 1, 2), 2, 2),
    # max_shift 4: three records at 4 are binned, two at 5 are not but count in n_in: 3 * 256 >= 128 * 5
    "shift_edge_inside": (16, 0, _EDGE, 4, 128, (4, 0, 4, 0, 5, 3, 5), 0, 2),
    # max_shift 3: no x bin holds anything, mode 0 with count 0, not supported
    "shift_edge_outside": (16, 0, _EDGE, 3, 128, (0, 0, 0, 0, 5, 0, 5), 2, 2),
    # margin 1: eight records at 9 in rows 0 and 5, four outside the grid; the three analysed ones move by 5.  Counted
    # with the others the mode would be 9 and the analysed cells (2, 2), (3, 2) would keep a residual of -4: 2 centres
    "margin_excluded": (16, 1, [(1, 0, 3, 9, 0), (2, 0, 3, 9, 0), (4, 5, 2, 9, 0), (9, 2, 2, 9, 0), (3, 7, 2, 9, 0),
                                (2, 2, 2, 5, 0), (3, 2, 1, 5, 0)], 16, 128, (5, 0, 5, 0, 3, 3, 3), 0, 2),
    # x: all four at 5.  y: 1, 2, 3, 4, one each: mode 1 (after 0 and -1 in the walk) with 1 * 256 < 128 * 4.  Threshold
    # 4: the residuals (0, dy) keep dy 2, 3, 4: (3, 2), (2, 3), (3, 3), each next to another: 3 (with gy 1: 2)
    "one_axis": (4, 0, [(2, 2, 1, 5, 1), (3, 2, 1, 5, 2), (2, 3, 1, 5, 3), (3, 3, 1, 5, 4)], 16, 128, (5, 0, 5, 1, 4, 4, 1), 3, 4),
    "no_records": (16, 0, [], 16, 128, (0, 0, 0, 0, 0, 0, 0), 0, 0),
    "max_shift_1": (1, 0, [(1, 1, 2, 1, 0), (2, 1, 1, 1, 0)], 1, 128, (1, 0, 1, 0, 3, 3, 3), 0, 2),
    # three at +127, two at -127: the residual of the two is -254, alone in (5, 4)
    "max_shift_127": (16, 0, [(1, 1, 2, 127, 0), (2, 1, 1, 127, 0), (5, 4, 2, -127, 0)], 127, 128, (127, 0, 127, 0, 5, 3, 5), 0, 2),
}
INFO_FIELDS = ("gx", "gy", "mode_x", "mode_y", "n_in", "n_x", "n_y")


def hand_frame(name):
    return voters(HAND[name][2], 4)


@functools.lru_cache(maxsize=None)
def hand_batches():
    """The cases grouped by what one call shares: [((thr, margin, max_shift, q8), names, mv, off, sd, want_centres,
    want_info rows, plain centres)].  Behind every case's frame stands a frame WITHOUT side data that owns records
    (a pan of 9): it reads 0 in every output."""
    return _batches(HAND)


def info_rows(info):
    """GMC_INFO_DTYPE [F] -> int64 [F, 7] in the order of INFO_FIELDS."""
    return np.stack([info[k].astype(np.int64) for k in INFO_FIELDS], axis=1)


# ------------------------------------------------------------------ a residual whose square needs more than 32 bits

# 32 x 32 cells of 1024 pixels (derived_edge_inputs.BIG_KW), margin 0, vectors_needed 1, max_shift 127.  Six records
# move by (-127, 0) in cell (5, 5): the mode, 6 * 256 >= 128 * 8; their residual is 0.  Cell (31, 31) holds one record with
# dx = 65535 (dst 32767, src -32768), dy = 0: residual 65535 + 127 = 65662, BIG_R2 = 65662^2 = 4 311 498 244 > 2^32
# (its low 32 bits are 16 530 948).  Column 31 is never a centre, so cell (30, 31) holds a helper with dx = 64511 (dst 31743,
# src -32768) and dy = 65535, not binned on y: |residual|^2 = 64638^2 + 65535^2 = 8 472 907 269, above every threshold
# used.  Cell (30, 31) is a centre iff the big record passes: 1, else 0.
BIG_R2 = 65662 * 65662
BIG_THRESHOLDS = [(4294967296.0, 1), (float(BIG_R2) - 0.5, 1), (float(BIG_R2), 1), (float(BIG_R2) + 1.0, 0)]
BIG_INFO = (-127, 0, -127, 0, 8, 6, 7)


@functools.lru_cache(maxsize=None)
def big_frame():
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    mv["dst_x"][:6], mv["dst_y"][:6] = 5 * 1024 + 512, 5 * 1024 + 512
    mv["src_x"][:6], mv["src_y"][:6] = 5 * 1024 + 512 + 127, 5 * 1024 + 512
    mv["dst_x"][6], mv["dst_y"][6], mv["src_x"][6], mv["src_y"][6] = 32767, 32767, -32768, 32767
    mv["dst_x"][7], mv["dst_y"][7], mv["src_x"][7], mv["src_y"][7] = 31743, 32767, -32768, -32768
    mv = mv[[3, 6, 0, 7, 1, 2, 4, 5]]
    return frozen(mv, np.array([0, 8], dtype=np.uint64), np.ones(1, dtype=np.uint8))


# ------------------------------------------------------------------ random pans on the 1080p grid

# Record counts that straddle the streamers' head (up to 15 records), step (4 x 1024 lanes) and tail; the frames follow
# one another without padding, so most frame starts are not 128-byte aligned in either layout.
PAN_COUNTS = [0, 1, 15, 16, 17, 4 * 1024 - 1, 4 * 1024, 4 * 1024 + 1]
PAN_MAX_SHIFT = 16


def pan_frame(rng, n, pan):
    """n records on 1920 x 1080: about two thirds carry the camera's `pan` anywhere in the picture (some outside it),
    the others move by up to +-10 inside six hot spots of 2 x 2 cells."""
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    if n == 0:
        return mv
    mover = rng.rand(n) < 0.34
    hot = rng.randint(0, 6, size=n)
    hx, hy = 200 + 290 * hot, 150 + 140 * hot
    dst_x = np.where(mover, hx + rng.randint(0, 32, size=n), rng.randint(-40, 1960, size=n))
    dst_y = np.where(mover, hy + rng.randint(0, 32, size=n), rng.randint(-40, 1120, size=n))
    dx = np.where(mover, rng.randint(-10, 11, size=n), pan[0])
    dy = np.where(mover, rng.randint(-10, 11, size=n), pan[1])
    mv["dst_x"], mv["dst_y"] = dst_x, dst_y
    mv["src_x"], mv["src_y"] = dst_x - dx, dst_y - dy
    mv["source"], mv["w"], mv["h"], mv["motion_scale"] = -1, 8, 8, 4
    return mv


@functools.lru_cache(maxsize=None)
def pan_batch():
    """(mv, off, sd, pans int64 [F, 2], shifts int64 [F, 2]): two frames per count of PAN_COUNTS, in a shuffled order,
    frames 5, 10 and 15 without side data; pans within +-6, and a translation (a, b) within +-4 per frame for consequence B."""
    rng = np.random.RandomState(20261019)
    counts = [c for c in PAN_COUNTS for _ in range(2)]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    pans = rng.randint(-6, 7, size=(len(counts), 2))
    frames = [pan_frame(rng, c, pans[i]) for i, c in enumerate(counts)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sd = np.ones(len(counts), dtype=np.uint8)
    sd[5::5] = 0
    shifts = rng.randint(-4, 5, size=(len(counts), 2))
    shifts[shifts.any(axis=1) == 0] = (3, -2)
    return frozen(np.concatenate(frames), off, sd, pans.astype(np.int64), shifts.astype(np.int64))


# ------------------------------------------------------------------ the pick across lanes and trips

# max_shift 127: 255 candidates; pick_mode gives lane l the walk indices l, l + 64, l + 128, l + 192.  Walk index -> value:
# 0 -> 0, 3 -> -2, 64 -> +32, 65 -> -33, 67 -> -34, 130 -> +65, 254 -> +127.  Three patterns of bin counts on an axis:
#   A   -2 (index 3: lane 3, trip 0), -34 (index 67: lane 3, trip 1) and +65 (index 130: lane 2, trip 2) tie: -2 wins
#   B   +127 (index 254: lane 62, trip 3) holds one record more than 0 (index 0: lane 0, trip 0): +127 wins
#   C   +32 (index 64: lane 0, trip 1) ties with -33 (index 65: lane 1, trip 1): +32 wins
# Each frame carries one pattern on x and another on y.  Same tuple as HAND; threshold 16, vectors_needed 1.  A group of
# records is laid out as a run of neighbouring cells in columns 1 .. 6, so it adds one centre per cell while its
# residual passes and nothing once the applied vector cancels it; a lone cell adds nothing either way.
_AB = [(1, 1, 2, -2, 127), (2, 1, 2, -2, 127),                                 # G1: the winner of both axes, 2 cells
       (4, 1, 2, -34, 127), (5, 1, 1, -34, 127), (6, 1, 1, -34, 127),          # G2: 3 cells
       (1, 4, 1, 65, 0), (2, 4, 1, 65, 0), (3, 4, 1, 65, 0), (4, 4, 1, 65, 0),  # G3: 4 cells
       (6, 3, 1, 1, 0), (7, 5, 1, 2, 0), (0, 3, 1, 3, 0)]                      # lone cells: dy 0 seven times, dy 127 eight
_BC = [(1, 1, 2, 127, 32), (2, 1, 1, 127, 32),                                 # H1: the winner of both axes, 2 cells
       (4, 1, 1, 127, -33), (5, 1, 1, 0, -33), (6, 1, 1, 0, -33),              # H2, H3: 3 cells in a row
       (6, 3, 1, 0, 5)]                                                        # dx 127 four times, 0 three times
_CA = [(1, 1, 1, 32, -2), (2, 1, 1, 32, -2),                                   # K1: the winner of both axes
       (4, 1, 1, -33, -34), (5, 1, 1, -33, -34),                               # K2
       (1, 4, 1, 7, 65), (2, 4, 1, 9, 65)]                                     # K3
LANES = {
    # x: A, y: B.  Applied (-2, 127): G1 cancels, G2 keeps (-32, 0): 3, G3 keeps (67, -127): 4.  With -34 on x: 2 + 0 + 4;
    # with +65: 2 + 3 + 4; with 0 on y: 2 + 3 + 4.  Unsupported from 69 on x (4 * 256 < 69 * 15) and from 137 on y
    # (8 * 256 = 2048 >= 136 * 15 = 2040 and < 137 * 15 = 2055); with gx 0 alone G1 keeps (-2, 0): 4 < 16, still nothing
    "lanes_A_on_x_B_on_y": (16, 0, _AB, 127, 0, (-2, 127, -2, 127, 15, 4, 8), 7, 9),
    "lanes_A_on_x_B_on_y_y_just_met": (16, 0, _AB, 127, 136, (0, 127, -2, 127, 15, 4, 8), 7, 9),
    "lanes_A_on_x_B_on_y_share_missed": (16, 0, _AB, 127, 137, (0, 0, -2, 127, 15, 4, 8), 9, 9),
    # x: B, y: C.  Applied (127, 32): H1 cancels, H2 + H3 keep (0, -65), (-127, -65): 3.  With 0 on x: 2 + 3; with -33 on
    # y: H1 keeps (0, 65): 2, H2 cancels, H3 keeps its two cells: 2.  x unsupported from 147 (4 * 256 = 1024 < 147 * 7 = 1029)
    "lanes_B_on_x_C_on_y": (16, 0, _BC, 127, 0, (127, 32, 127, 32, 7, 4, 3), 3, 5),
    "lanes_B_on_x_C_on_y_share_missed": (16, 0, _BC, 127, 147, (0, 0, 127, 32, 7, 4, 3), 5, 5),
    # x: C, y: A.  Applied (32, -2): K1 cancels, K2 keeps (-65, -32): 2, K3: 2.  Any other winner on either axis leaves a
    # residual of 32 or more on K1: 6.  Unsupported from 86 (2 * 256 = 512 < 86 * 6 = 516)
    "lanes_C_on_x_A_on_y": (16, 0, _CA, 127, 0, (32, -2, 32, -2, 6, 2, 2), 4, 6),
    "lanes_C_on_x_A_on_y_share_missed": (16, 0, _CA, 127, 86, (0, 0, 32, -2, 6, 2, 2), 6, 6),
}
LANE_WALK = {-2: 3, -34: 67, 65: 130, 127: 254, 0: 0, 32: 64, -33: 65}          # value -> walk index, as stated above


def _batches(cases):
    groups = {}
    for name, (thr, margin, _cells, ms, q8, _info, _c, _pl) in cases.items():
        groups.setdefault((thr, margin, ms, q8), []).append(name)
    out = []
    for key, names in groups.items():
        frames, sd, centres, info, plain = [], [], [], [], []
        rng = np.random.RandomState(len(out) + 17)
        for n in names:
            f = voters(cases[n][2], 4)
            frames += [f[rng.permutation(len(f))], voters(_pan(9, 0), 4)]
            sd += [1, 0]
            centres += [cases[n][6], 0]
            info += [cases[n][5], (0,) * 7]
            plain += [cases[n][7], 0]
        off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
        arrays = frozen(np.concatenate(frames), off, np.array(sd, dtype=np.uint8), np.array(centres, dtype=np.uint32),
                        np.array(info, dtype=np.int64), np.array(plain, dtype=np.uint32))
        out.append((key, tuple(names)) + arrays)
    return out


@functools.lru_cache(maxsize=None)
def lane_batches():
    """LANES in the form of hand_batches(): one batch per setting, a pan of 9 without side data behind every case."""
    return _batches(LANES)


# ------------------------------------------------------------------ has_sd == NULL: the frame owns no record

def follower_by_hand(margin, ms):
    """(centres, info) of hand_batches()' frames WITHOUT side data once has_sd is NULL and they are scanned: one record
    per cell moving by (9, 0).  Within max_shift the pan is found, fully supported (every counted record) and cancelled;
    beyond it no x bin holds anything, nothing is applied and all 8 x (6 - 2 margin) analysed cells are active: columns
    1 .. 6 of them are centres."""
    n = GW * (GH - 2 * margin)
    if ms >= 9:
        return 0, (9, 0, 9, 0, n, n, n)
    return (GW - 2) * (GH - 2 * margin), (0, 0, 0, 0, n, 0, n)


# ------------------------------------------------------------------ 2^24 records in a frame

# The smallest frame at which the support test and the pick's key differ from 32-bit arithmetic.  2^24 + 1 records move
# by (5, -3), alternating between cells (1, 1) and (2, 1); the last record of the frame, in (2, 1), moves by (6, -3).
# n_in = 2^24 + 2, n_x = 2^24 + 1, n_y = n_in.  min_share_q8 256: n_x * 256 = 2^32 + 256 < 256 * n_in = 2^32 + 512: x is
# not supported, gx 0, the residuals (5, 0) and (6, 0) pass 16, both cells are active neighbours in inner columns: 2.
# In 32 bits the two sides read 256 and 512 (still unsupported) if BOTH wrap, but `n_x << 8` alone wrapping, or the
# pick's count << 8 losing its top bits, gives other answers; 255: 255 * n_in = 2^32 - 2^24 + 510 <= n_x * 256: supported,
# gx 5, the residuals are (0, 0) and (1, 0): 0.
HUGE_N = 2 ** 24 + 2
HUGE_TRIPLE = [(1, 1, 1, 5, -3), (2, 1, 1, 5, -3), (2, 1, 1, 6, -3)]            # the records A, B and the odd one
HUGE = {256: ((0, -3, 5, -3, HUGE_N, HUGE_N - 1, HUGE_N), 2), 255: ((5, -3, 5, -3, HUGE_N, HUGE_N - 1, HUGE_N), 0)}


# ------------------------------------------------------------------ more frames than one trip of the clear kernels

CLEAR_TRIP = 1024 * 256               # lanes of gmc_clear_kernel, zones_clear_kernel and blobs_clear_kernel: one element each
CLEAR_FRAMES = CLEAR_TRIP + 300
CLEAR_CASE = "pan_plus_object"        # compensated: 4 centres, info (5, 0, 5, 0, 48, 44, 48); plain: 36, one blob of 6 x 6
CLEAR_BOX = (1, 0, 6, 5)              # the plain scan's centres: columns 1 .. 6 of every row, one component of 36 cells


@functools.lru_cache(maxsize=None)
def clear_batch():
    """(mv, off, sd, planted frame indices): CLEAR_FRAMES frames that own no record and have no side data, but CLEAR_CASE
    at frames 0, CLEAR_TRIP - 1, CLEAR_TRIP (the first element of the clear's second trip) and the last one, and frames
    WITHOUT side data that own a pan of 9 next to them: 1, CLEAR_TRIP + 1 and the one before the last (CLEAR_TRIP - 1
    and CLEAR_TRIP are neighbours: the frame behind the two serves both)."""
    planted = (0, CLEAR_TRIP - 1, CLEAR_TRIP, CLEAR_FRAMES - 1)
    pans = (1, CLEAR_TRIP + 1, CLEAR_FRAMES - 2)
    counts = np.zeros(CLEAR_FRAMES, dtype=np.int64)
    one, pan = hand_frame(CLEAR_CASE), voters(_pan(9, 0), 4)
    counts[list(planted)], counts[list(pans)] = len(one), len(pan)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    mv = np.concatenate([one if f in planted else pan for f in sorted(planted + pans)])
    sd = np.zeros(CLEAR_FRAMES, dtype=np.uint8)
    sd[list(planted)] = 1
    return frozen(mv, off, sd) + (planted,)


# ------------------------------------------------------------------ a host batch that does not start at record 0

REBASE = 4097


@functools.lru_cache(maxsize=None)
def embedded_pan_batch():
    """(mv, off): pan_batch()'s records behind REBASE records that move by up to +-40 in the picture's middle and in front
    of 1000 more of them; off = pan_batch()'s + REBASE.  A scan that read from record 0, or past off[-1], would count them."""
    mv, off, sd, _, _ = pan_batch()
    rng = np.random.RandomState(7)
    pad = np.zeros(REBASE + 1000, dtype=m.MV_DTYPE)
    pad["dst_x"], pad["dst_y"] = rng.randint(600, 1300, size=len(pad)), rng.randint(300, 800, size=len(pad))
    pad["src_x"], pad["src_y"] = pad["dst_x"] - rng.randint(-40, 41, size=len(pad)), pad["dst_y"] - rng.randint(-40, 41, size=len(pad))
    return frozen(np.concatenate([pad[:REBASE], mv, pad[REBASE:]]), (off + np.uint64(REBASE)).astype(np.uint64))
