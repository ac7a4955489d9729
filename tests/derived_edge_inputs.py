"""Inputs of tests/test_gpu_derived_edges.py: the record-level and plan-level edge cases of the scan's suite, rebuilt for
the kernels that stream records with csrc/record_stream.h's shared streamers as each of them instantiates them
(sweep_frames_kernel, activity_frames_kernel) or with a loop of their own (motion_scores_kernel).  Every builder returns its input together with the values derived BY HAND from its construction;
tests/test_derived_edges_host.py checks those against the oracle (and the numpy model of the maps) without a GPU, and
that the plans reach the forms the GPU tests rely on.  Everything is built once per process and handed out read-only."""
import functools
import math

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import synth

import oracle_binding as ob
from golden_cases import build_mvs, load_hand_cases
from scan_checks import junk_padding
from test_gpu_parity import BIG_D, test_scan_magnitude_beyond_32_bits as _scan_big_test

MI355X_LDS = 163840
INF = float("inf")


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def voters(cells, shift=4):
    """cells = [(gx, gy, votes, dx, dy)] -> one record per vote, dst in the middle of the cell, dst - src = (dx, dy)."""
    n = sum(c[2] for c in cells)
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    at = 0
    half = (1 << shift) >> 1
    for gx, gy, votes, dx, dy in cells:
        s = slice(at, at + votes)
        mv["dst_x"][s], mv["dst_y"][s] = (gx << shift) + half, (gy << shift) + half
        mv["src_x"][s], mv["src_y"][s] = (gx << shift) + half - dx, (gy << shift) + half - dy
        at += votes
    return mv


def batch_of(frames, seed):
    """Frames (record arrays) -> (mv, off, sd): the records of each frame shuffled, junk in the padding bytes."""
    rng = np.random.RandomState(seed)
    b = m.FrameBatch.from_frames([f[rng.permutation(len(f))] for f in frames])
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    return mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), np.ones(len(frames), dtype=np.uint8)


def sweep_tile_bytes(p):
    """csrc/sweep_kernels.h, sweep_tile_words: (analysed rows + 2) x grid_w 32-bit counters, padded to 16 bytes."""
    R = max(1, max(p.grid_h - p.vertical_margin, p.vertical_margin) - p.vertical_margin)
    return 4 * (((R + 2) * p.grid_w + 3) & ~3), R


def sweep_chunk_rows(p, n_thr, n_vec, lds=MI355X_LDS):
    """(chunk_rows, R, single): the centre rows per phase-2 chunk that mtgpu_scan_sweep_preview's lds_bytes stands for
    (lds_bytes = per_pass x tile + n_vec x (chunk_rows + 2) x W x 8 + 256), and what one chunk of all R rows would take."""
    pv = m.sweep_preview(p, n_thr, n_vec, lds)
    tile, R = sweep_tile_bytes(p)
    W = (p.grid_w + 63) // 64
    rest = pv["lds_bytes"] - pv["thresholds_per_pass"] * tile - 256
    assert rest > 0 and rest % (n_vec * W * 8) == 0, (pv, tile)
    single = pv["thresholds_per_pass"] * tile + n_vec * (R + 2) * W * 8 + 256
    return rest // (n_vec * W * 8) - 2, R, single, pv


# ------------------------------------------------------------------ A. every pass shape of the sweep

# |dx|, |dy| <= 6 in synth.random_frames: |d|^2 is a sum of two squares in 0 .. 72.  Between any two neighbours of this
# list lies one (2 | 5 8 9 | 10 13 16 | 17 .. 25 | 26 .. 36 | 37 .. 45 | 50 52 | 61 72), so the eight settings differ.
THR8 = [2, 5, 10, 17, 26, 37, 50, 61]
VEC8 = [1, 2, 3, 4, 5, 6, 7, 8]

# name: (width, height, thresholds in the CALLER's order, vector levels, (passes, thresholds per pass) at 163 840 B)
PASS_SHAPES = {
    "1080p-1of-multi-tile": (1920, 1080, [17], [2, 4], (1, 1)),                        # NT 1, fold skipped
    "1080p-2": (1920, 1080, [26, 5], [8, 1, 4, 2], (1, 2)),                            # NT 2
    "1080p-5": (1920, 1080, [26, 2, 50, 10, 37], [4, 1, 2], (1, 5)),                   # NT 8, three pads
    "1080p-4+3-specials": (1920, 1080, [10, INF, 2, 26, 10, 0.0, 50], [1, 2, 3], (2, 4)),   # NT 4 full, NT 4 with a pad
    "720p-6-three-levels": (1280, 720, [37, 5, 61, 2, 17, 50], [1, 3, 6], (1, 6)),     # NT 8, two pads
    "720p-7": (1280, 720, [50, 10, 2, 61, 26, 5, 37], [5, 2], (1, 7)),                 # NT 8, one pad
    "720p-8x8": (1280, 720, [26, 61, 2, 37, 10, 50, 5, 17], [3, 8, 1, 6, 2, 7, 4, 5], (1, 8)),   # NT 8 full, 64 settings
    "1080p-8x8": (1920, 1080, [37, 2, 61, 10, 50, 5, 26, 17], VEC8, (2, 4)),           # 4 + 4, 64 settings
}


@functools.lru_cache(maxsize=None)
def pass_shape_frames(width, height):
    """16 (1080p) / 12 (720p) random ragged frames of up to 3000 records, junk in the padding bytes."""
    rng = np.random.RandomState(width + height)
    mv, off, sd = synth.random_frames(rng, 16 if width == 1920 else 12, 3000, width, height)
    junk_padding(mv, rng)
    return frozen(mv, off, sd)


@functools.lru_cache(maxsize=None)
def _oracle_setting(width, height, thr, vec):
    mv, off, sd = pass_shape_frames(width, height)
    p = ob.params_from_config(width, height, mv_threshold_sq=thr, vectors_needed=vec)
    return frozen(ob.scan_centres(p, mv, off, sd, nthreads=4)[1])[0]


def pass_shape_case(name):
    """(params, mv, off, sd, thresholds, vectors, plan, oracle block uint32 [T, V, F]): one oracle pass per distinct
    setting, shared by the cases of a grid."""
    width, height, thr, vec, plan = PASS_SHAPES[name]
    mv, off, sd = pass_shape_frames(width, height)
    want = np.stack([np.stack([_oracle_setting(width, height, float(t), int(v)) for v in vec]) for t in thr])
    return m.ScanParams.from_config(width, height), mv, off, sd, thr, vec, plan, want


# ------------------------------------------------------------------ B. chunk seams of the sweep's phase 2

# name: (width, height, thresholds in the caller's order, chunk_rows at 163 840 B)
SEAM_GRIDS = {"64x600": (1024, 9600, [25, 9], 146), "4k": (3840, 2160, [25], 123)}
SEAM_KW = dict(vertical_mask=0.0)


def seam_pairs(gw, gh):
    """Frame 0: the even y, frame 1: the odd y of [0, gh - 2].  Pair y = cells (x, y) and (x, y + 1), x stepping by 3
    modulo gw - 2 inside [1, gw - 2]: the pairs of a frame are two rows apart and never in neighbouring columns, so
    each cell's only active neighbour is the other cell of its pair.  k = 1 + y % 8 votes per cell; |d|^2 = 25 where
    y // 8 is even, else 9."""
    frames = [[], []]
    for y in range(gh - 1):
        frames[y % 2].append((1 + (3 * (y // 2)) % (gw - 2), y, 1 + y % 8, 5 if (y // 8) % 2 == 0 else 3))
    return frames


def seam_row_pairs(gw, ch):
    """The third frame: horizontal pairs (x, x + 1) on the last row of the first chunk — across every 64-bit word
    boundary the grid has, in the last two columns where it has none — and one pair on the first row of the second
    chunk.  [(x, y, k, centres of the pair)]: a cell in column gw - 1 is never a centre."""
    row = [(63, ch - 1, 2, 2), (127, ch - 1, 5, 2), (191, ch - 1, 8, 2)] if gw == 240 else [(30, ch - 1, 5, 2), (gw - 2, ch - 1, 8, 1)]
    return row + [(10, ch, 4, 2)]


@functools.lru_cache(maxsize=None)
def seam_case(name):
    """(params, mv, off, sd, thresholds, vectors, hand block uint32 [T, 8, 3])."""
    width, height, thr, ch = SEAM_GRIDS[name]
    p = m.ScanParams.from_config(width, height, **SEAM_KW)
    gw, gh = p.grid_w, p.grid_h
    pairs = seam_pairs(gw, gh)
    rows = seam_row_pairs(gw, ch)
    frames = [voters([(x, y + j, k, d, 0) for x, y, k, d in fr for j in (0, 1)]) for fr in pairs]
    frames.append(voters([(x + j, y, k, 5, 0) for x, y, k, _ in rows for j in (0, 1)]))
    mv, off, sd = batch_of(frames, gw)
    hand = np.zeros((len(thr), 8, 3), dtype=np.uint32)
    for t, T in enumerate(thr):
        for v, V in enumerate(VEC8):
            for f in (0, 1):
                hand[t, v, f] = 2 * sum(1 for x, y, k, d in pairs[f] if k >= V and d * d >= T)
            hand[t, v, 2] = sum(c for x, y, k, c in rows if k >= V and 25 >= T)
    return (p,) + frozen(mv, off, sd) + (thr, VEC8) + frozen(hand)


# ------------------------------------------------------------------ C. |d|^2 at and above 2^32

BIG_THRESHOLDS = list(_scan_big_test.pytestmark[0].args[1])          # the ten thresholds of the scan's test
BIG_KW = dict(block_size=1024, block_shift=10, vertical_mask=0.0)
# The scan's test puts the two records of a BIG_D pair into two neighbouring 16-pixel cells.  On a grid the derived
# kernels support a cell is at least 256 pixels wide, and a record with |dx| >= 65 519 has dst_x >= 32 751: both records
# of a pair fall into the LAST column (31) of the last row, which is never a centre.  So column 30 of that row gets two
# helper records with the largest magnitude a record of that column can have (dst 31 743, src -32 768; dst_y 32 767,
# src_y -32 768), and the two vector levels tell "one" from "both": column 30 is a centre at level v iff the helpers
# pass the threshold and at least v of the pair's two magnitudes do.
BIG_HELPER = 64511 * 64511 + 65535 * 65535                           # 8 456 505 346 > 2^32


def big_passes(D, thr):
    return D >= math.ceil(thr)


@functools.lru_cache(maxsize=None)
def big_frames():
    """(mv, off, sd): five frames, one per BIG_D pair — its two records in cell (31, 31), two helpers in (30, 31)."""
    frames = []
    for da, db in BIG_D:
        mv = np.zeros(4, dtype=m.MV_DTYPE)
        mv["dst_x"], mv["dst_y"] = [32767, 32751, 31743, 31743], 32767
        mv["src_x"] = [32767 - da[0], 32751 - db[0], -32768, -32768]
        mv["src_y"] = [32767 - da[1], 32767 - db[1], -32768, -32768]
        frames.append(mv)
    b = m.FrameBatch.from_frames(frames)
    return frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy(), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
                  np.ones(5, dtype=np.uint8))


def big_hand_count(thr, level):
    """Centre count per frame from exact Python integers: 1 iff the helpers and >= level of the pair's records pass."""
    return [int(big_passes(BIG_HELPER, thr) and sum(big_passes(dx * dx + dy * dy, thr) for dx, dy in pair) >= level)
            for pair in BIG_D]


# two calls of five thresholds, each in an order that is neither ascending nor descending
BIG_CALLS = [[BIG_THRESHOLDS[i] for i in (2, 0, 4, 1, 3)], [BIG_THRESHOLDS[i] for i in (7, 9, 5, 8, 6)]]
BIG_ACTIVITY_THRESHOLDS = [4294836225.5, 4294967296.0, 8589672450.5]


# ------------------------------------------------------------------ D. head, step boundary and tail

STEP40, STEP8 = 1024 * 4, 1024 * 4 * 2          # records per step of the unrolled loop: kSweepBlock x kSweepUnroll (pairs on compact)
EDGE_THR, EDGE_VEC = [1, 4, 6], [3, 4]
BIG_KINDS = [STEP40 - 1, STEP40, STEP40 + 1, STEP8 - 1, STEP8, STEP8 + 1, STEP8 + 2,
             2 * STEP8 - 1, 2 * STEP8, 2 * STEP8 + 1, 2 * STEP8 + 2]      # 2 x STEP40 == STEP8


def head_of(off):
    """Records the kernels peel ahead of the first 128-byte line when the record array starts on one: 40 h = -40 off and
    8 h = -8 off (mod 128) have the same solution h < 16."""
    return (16 - int(off) % 16) % 16


def _edge_cells(idx):
    """Cell A and its 4-neighbour N of test frame idx: inner columns, analysed rows."""
    ax, ay = 2 + (idx * 7) % 114, 5 + (idx * 11) % 56
    return (ax, ay), [(ax + 1, ay), (ax, ay + 1), (ax - 1, ay), (ax, ay - 1)][idx % 4]


def _filler(n, rng, first, last):
    """n >= 2 still records; the first one votes (|d|^2 = 5) into cell `first`, the last one into cell `last`: one vote
    in a frame of its own makes no cell active at level 3, but a neighbouring frame that reads one record too many
    gives its cell A a fourth voter."""
    f = np.zeros(n, dtype=m.MV_DTYPE)
    f["dst_x"], f["dst_y"] = rng.randint(0, 1920, size=n), rng.randint(0, 1080, size=n)
    f["src_x"], f["src_y"] = f["dst_x"], f["dst_y"]
    for q, cell in ((0, first), (n - 1, last)):
        if cell is not None:
            f["dst_x"][q], f["dst_y"][q] = cell[0] * 16 + 8, cell[1] * 16 + 8
            f["src_x"][q], f["src_y"][q] = cell[0] * 16 + 7, cell[1] * 16 + 6
    return f


def _edge_frame(n, h, idx, rng):
    """n records with zero displacement (they pass no threshold >= 1) but 13 (fewer in a frame shorter than 13): cell A
    gets EXACTLY 3 voters with |d|^2 = 5 on the positions a wrong loop bound would drop or read twice, its neighbour N
    gets min(10, n - 3) >= 4 on positions in between."""
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = rng.randint(0, 1920, size=n), rng.randint(0, 1080, size=n)
    mv["src_x"], mv["src_y"] = mv["dst_x"], mv["dst_y"]
    cand = []
    for q in (0, h - 1, h, h + 1023, h + 1024, h + STEP40 - 1, h + STEP40, h + STEP8 - 1, h + STEP8, n - 2, n - 1):
        if 0 <= q < n and q not in cand:
            cand.append(q)
    rot = idx % len(cand)
    a_pos = (cand[rot:] + cand[:rot])[:3]
    free = [q for q in range(min(n, 64))] + list(range(64, n, max(1, n // 997)))
    free = [q for q in free if q not in a_pos]
    n_n = min(10, n - 3)
    n_pos = [free[(2 * j + 1) * len(free) // (2 * n_n)] for j in range(n_n)]
    assert len(a_pos) == 3 and len(set(n_pos)) == n_n >= 4 and not set(n_pos) & set(a_pos)
    (ax, ay), (nx, ny) = _edge_cells(idx)
    for pos, (gx, gy), (dx, dy) in ((a_pos, (ax, ay), (1, 2)), (n_pos, (nx, ny), (2, -1))):
        mv["dst_x"][pos], mv["dst_y"][pos] = gx * 16 + 8, gy * 16 + 8
        mv["src_x"][pos], mv["src_y"][pos] = gx * 16 + 8 - dx, gy * 16 + 8 - dy
    return mv, (ax, ay), (nx, ny), a_pos


@functools.lru_cache(maxsize=None)
def edge_batch():
    """(mv, off, sd, test: frame indices, cells: {frame: (A, N)}, lengths: {frame: (head, n)}).  68 test frames on
    1920x1080, each between two filler frames of 2 .. 17 still records; the one in front puts the test frame's first
    record on the wanted residue of a 128-byte line, and the records next to a test frame vote into its cell A (see
    _filler).  Every head 8 .. 15 with a frame one record shorter than, as long as and one longer than the head (a
    shorter head cannot hold the voters), and every residue with frames of head + BIG_KINDS."""
    rng = np.random.RandomState(44)
    want = []                                              # (residue of the first record, length - head)
    big = [(j % 16, BIG_KINDS[j % 11]) for j in range(44)]
    small = [(o, d) for o in range(1, 9) for d in (-1, 0, 1)]
    while big or small:
        if big:
            want.append(big.pop(0))
        if small:
            want.append(small.pop(0))
    frames, test, cells, lengths, at = [], [], {}, {}, 0
    for idx, od in enumerate(want + [None]):
        o, d = od if od else (None, None)
        fill = 2 if o is None else (o - at) % 16 + (16 if (o - at) % 16 < 2 else 0)
        frames.append(_filler(fill, rng, _edge_cells(idx - 1)[0] if idx else None, None if o is None else _edge_cells(idx)[0]))
        at += fill
        if o is None:
            break
        h = head_of(at)
        assert at % 16 == o
        mv, a, nb, _ = _edge_frame(h + d, h, idx, rng)
        test.append(len(frames))
        cells[len(frames)], lengths[len(frames)] = (a, nb), (h, h + d)
        frames.append(mv)
        at += h + d
    b = m.FrameBatch.from_frames(frames)
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    return frozen(mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), np.ones(len(frames), dtype=np.uint8)) + \
        (tuple(test), cells, lengths)


def edge_hand_sweep():
    """uint32 [3, 2, F] for EDGE_THR x EDGE_VEC: A (3 voters) and N are both active at level 3 under thresholds 1 and 4 and
    neighbours: 2; at level 4 only N is active: 0; nothing passes threshold 6; a filler frame holds at most two voters, one per cell."""
    _, off, _, test, _, _ = edge_batch()
    hand = np.zeros((3, 2, len(off) - 1), dtype=np.uint32)
    hand[:2, 0, list(test)] = 2
    return hand


EDGE_STREAMS = (0, 37)                                     # two streams: frames [0, 37) and [37, F)


def edge_hand_maps(vectors_needed):
    """(active, centre, frames) uint32 [2, 68, 120] x 2, [2]: per test frame A and N active and centres at 3, only N
    active and no centre at 4; every frame has side data and contributes (min_centres 0)."""
    _, off, _, test, cells, _ = edge_batch()
    F = len(off) - 1
    soff = list(EDGE_STREAMS) + [F]
    active, centre = np.zeros((2, 68, 120), dtype=np.uint32), np.zeros((2, 68, 120), dtype=np.uint32)
    for f in test:
        s = 0 if f < soff[1] else 1
        (ax, ay), (nx, ny) = cells[f]
        active[s, ny, nx] += 1
        if vectors_needed == 3:
            active[s, ay, ax] += 1
            centre[s, ay, ax] += 1
            centre[s, ny, nx] += 1
    return active, centre, np.array([soff[1], F - soff[1]], dtype=np.uint32), np.array(soff, dtype=np.uint64)


# ------------------------------------------------------------------ E. 4-byte-aligned 40-byte bases

UNALIGNED_SHIFTS = (4, 12, 20)


@functools.lru_cache(maxsize=None)
def unaligned_batch():
    rng = np.random.RandomState(45)
    mv, off, sd = synth.random_frames(rng, 40, 2500, 1920, 1080)
    junk_padding(mv, rng)
    return frozen(mv, off, sd)


# ------------------------------------------------------------------ F. the 16-bit accumulator boundary

ACC_FRAMES, ACC_SPLIT = 70000, 65535


@functools.lru_cache(maxsize=None)
def acc_batch():
    """70 000 frames of the same four records: two votes into cell (40, 30), two into (41, 30) of the 1080p grid — both
    active and centres in every frame under the defaults (VECTORS_NEEDED 2, |d|^2 = 25 >= 16)."""
    one = voters([(40, 30, 2, 5, 0), (41, 30, 2, 3, 4)])
    mv = np.ascontiguousarray(np.tile(one, ACC_FRAMES), dtype=m.MV_DTYPE)
    off = np.arange(ACC_FRAMES + 1, dtype=np.uint64) * 4
    return frozen(mv, off, np.ones(ACC_FRAMES, dtype=np.uint8))


def acc_hand(counts):
    """(active, centre, frames) for streams that hold `counts` frames each."""
    plane = np.zeros((len(counts), 68, 120), dtype=np.uint32)
    for s, n in enumerate(counts):
        plane[s, 30, 40:42] = n
    return plane, plane.copy(), np.array(counts, dtype=np.uint32)


# ------------------------------------------------------------------ G. the hand-derived check_frame goldens

def hand_case_batch(case):
    """(mv, off, sd, hand centre count) of one case of tests/golden/check_frame_hand_cases.json."""
    mv = build_mvs(case)
    sd = int(case.get("has_sd", 1))
    return mv, np.array([0, len(mv)], dtype=np.uint64), np.array([sd], dtype=np.uint8), (case["centres"] if sd else 0)


def hand_case_settings(kw):
    return [INF, kw["mv_threshold_sq"], 0.0], [255, kw["vectors_needed"], 0]


def hand_base_batch():
    """The cases that share the base parameters as one batch: (base kwargs, mv, off, sd, hand counts)."""
    g, cases = load_hand_cases()
    base = [c for _, kw, c in cases if kw == g["base"]]
    frames = [build_mvs(c) for c in base]
    sd = np.array([int(c.get("has_sd", 1)) for c in base], dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    mv = np.zeros(int(off[-1]), dtype=m.MV_DTYPE)
    for i, f in enumerate(frames):
        mv[int(off[i]):int(off[i + 1])] = f
    return g["base"], mv, off, sd, [c["centres"] if s else 0 for c, s in zip(base, sd)]
