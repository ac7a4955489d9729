"""Inputs of tests/test_gpu_pipe_lanes.py (direction planes carried through the pipe, under its keep mask;
include/mtgpu_pipe_lanes.h), built once and frozen, and the model.  The model states consequence P4 of the header
literally and adds nothing of its own:

    centres      remove every record whose sector its destination cell forbids (lanes_model.filter_records' rule, with the
                 ONE plane) -> the masked plain pipe (pipe_gmc_inputs.masked_plain through pipe_dir_inputs: the zones
                 model's AND rule; no keep plane: the plain scan)
    sector word  remove every record of a keep-0 cell (pipe_dir_inputs.remove_masked) -> the rose of tests/dir_model.py ->
                 direction.sector_word

tests/test_pipe_lanes_host.py checks, without a GPU, that the model returns every hand-derived number below and that it
agrees with the unchanged oracle through removal on every input.  Frames are lists; None is a frame without side data.
No GPU and no library call in this file beyond the previews (host arithmetic)."""
import dataclasses
import functools

import numpy as np

import mvtrim_amd as m

import derived_cliff_inputs as dc
import dir_inputs as di
import lanes_inputs as li
import lanes_model as lm
import oracle_binding as ob
import pipe_dir_inputs as pd
import pipe_gmc_inputs as pg
from derived_edge_inputs import frozen, voters

E, SE, S, SW, W, NW, N, NE = range(8)
word = pd.word


# ------------------------------------------------------------------ the model

def remove_forbidden(p, frames, plane):
    """The frames without the records whose sector their destination cell's byte forbids: lanes_model.filter_records with
    the one plane (None stays None).  filter_records joins its parts with np.concatenate, which packs the 40-byte records
    into 32 bytes (docs/rounds/r21_pipe_dir.md): its answer says WHICH records stay, and FrameBatch.from_frames lays each
    frame out again as 40-byte records."""
    parts = [np.zeros(0, dtype=m.MV_DTYPE) if f is None else f for f in frames]
    b = m.FrameBatch.from_frames(parts)
    fmv, foff = lm.filter_records(p, b.mv, b.frame_off, plane)
    out = []
    for i, f in enumerate(frames):
        part = m.FrameBatch.from_frames([fmv[int(foff[i]):int(foff[i + 1])]]).mv
        assert part.dtype == m.MV_DTYPE and part.dtype.itemsize == 40
        out.append(None if f is None else part)
    return out


def sector_words(p, frames, keep=None):
    return pd.sector_words(p, frames, keep)


def model(p, frames, plane, keep=None):
    """(flags, centres, sector words) lists of the plane pipe on `frames`."""
    fl, ce = pg.masked_plain(p, remove_forbidden(p, list(frames), plane), keep)
    return fl, ce, sector_words(p, frames, keep)


def oracle_centres(p, frames, plane, keep=None):
    """The same centres from the unchanged oracle, through removal: the forbidden records out and, under a keep plane,
    the records of keep-0 cells out as well — with vectors_needed >= 1 a cell without a vote is inactive, exactly as a
    cell whose keep bit is 0 (vectors_needed == 0 has no such removal: every cell is active without a vote)."""
    assert keep is None or p.vectors_needed >= 1
    parts = []
    for f, g in zip(frames, remove_forbidden(p, list(frames), plane)):
        g = np.zeros(0, dtype=m.MV_DTYPE) if f is None else g
        parts.append(g if keep is None else pd.remove_masked(p, g, keep))
    b = m.FrameBatch.from_frames(parts)
    sd = np.array([f is not None for f in frames], dtype=np.uint8)
    return ob.scan_centres(p, b.mv, b.frame_off, sd, nthreads=4)[1].tolist()


def case_frames(case):
    """A lanes_inputs case -> its frames as a list (None: no side data)."""
    return pd.case_frames(case)


def filled(p, byte):
    return frozen(np.full((p.grid_h, p.grid_w), byte, dtype=np.uint8))[0]


# ------------------------------------------------------------------ 1. the hand cases of lanes_inputs through a pipe

def hand_rows(name):
    """[(frame, plane, centres, rose)] of lanes_inputs.HAND_CASES[name]: each of its streams holds one frame, so frame f
    goes through a pipe under plane f.  The documented values: one_cell 2 / 0 / 0 with rose 3 E / 1 W; neighbours
    0 / 2 / 0; still 2 and 3; vn0 20, 20, 20; margin 2 and 2."""
    c = li.HAND_CASES[name]()
    frames = case_frames(c)
    assert len(frames) == len(c["planes"]) == len(c["soff"]) - 1
    return c["params"], [(frames[f], c["planes"][f], int(c["hand_centres"][f]), [int(x) for x in c["hand_rose"][f]])
                         for f in range(len(frames))]


HAND_DOCUMENTED = {"one_cell": [2, 0, 0], "neighbours": [0, 2, 0], "still": [2, 3], "vn0": [20, 20, 20], "margin": [2, 2]}


# ------------------------------------------------------------------ 2. two lanes and a clock, by hand

@functools.lru_cache(maxsize=None)
def two_lane_case():
    """(params, frame, plane, keep, (centres, word) without the mask, (centres, word) with it) on the 6 x 5 grid (16-pixel
    cells, threshold 4, one vote makes a cell active, one centre a flag, no margin; columns 1 .. 4 can be centres).
      plane   rows 1 and 3 hold W alone (0x10), every other row 0xFF: a road whose two lanes both run west.
      frame   row 1: (1, 1) and (2, 1), one record each, moving EAST: their cells allow only W, they do not vote.
              row 3: (1, 3) and (2, 3), one record each, moving WEST: they vote, each has an active neighbour.
              row 0: (3, 0) and (4, 0), one record each, moving SOUTH: the burnt-in clock; its cells hold 0xFF, they vote.
      keep    clears the rectangle (3, 0) .. (4, 0).
    No mask: active (1, 3), (2, 3), (3, 0), (4, 0), every one with an active neighbour and in columns 1 .. 4 (row 1 under
    the clock is inactive): 4 centres.  n[E] = 2, n[S] = 2, n[W] = 2: present 0x15, the tie goes to the smallest k = E,
    count 2.
    Mask: the clock's records do not count and its cells are inactive: 2 centres.  n[E] = 2, n[W] = 2: present 0x11,
    dominant E, count 2.
    A build that read one byte for the whole picture could not give 4 and 2: under 0x10 the clock would not vote (2 and
    2), under 0xFF the E pair would (6 and 4)."""
    p = pd.small_params()
    fr = voters([(1, 1, 1, 5, 0), (2, 1, 1, 5, 0), (1, 3, 1, -5, 0), (2, 3, 1, -5, 0), (3, 0, 1, 0, 5), (4, 0, 1, 0, 5)])
    fr = fr[np.random.RandomState(26).permutation(len(fr))]
    plane = np.full((5, 6), 0xFF, dtype=np.uint8)
    plane[1], plane[3] = 1 << W, 1 << W
    keep = pd.small_keep([(3, 0), (4, 0)])
    return p, frozen(fr)[0], frozen(plane)[0], keep, (4, word(0x15, E, 2)), (2, word(0x11, E, 2))


# ------------------------------------------------------------------ 3. P1 - P6: every layout and batch geometry

SHAPE_BYTES = [0xFF, 0x5B, 0x01, 0x00]                 # P3: a plane filled with one byte == the direction pipe under it


@functools.lru_cache(maxsize=None)
def shapes_case():
    """pipe_dir_inputs.shapes_case() — 14 frames on the 80 x 6 grid, vectors_needed 2: frames without side data first,
    interleaved and last, an empty frame, one of 4 097 records, one of a single record; keep with 25 % of the cells
    cleared — with a random plane, and a plane whose bits are a subset of it in every cell (P6)."""
    p, frames, keep = pd.shapes_case()
    rng = np.random.RandomState(2600)
    a = rng.randint(0, 256, size=(p.grid_h, p.grid_w)).astype(np.uint8)
    b = a & rng.randint(0, 256, size=a.shape).astype(np.uint8)
    return p, frames, keep, frozen(a)[0], frozen(b)[0]


# ------------------------------------------------------------------ 4. word seams and the copy's byte phase

def seam_params(gw, margin):
    """lanes_inputs.seam_case(gw)'s grid, gw x 9 cells; margin 1: rows 1 .. 7 are analysed — every record of the case lies
    in them — and y_lo gw is odd: the staged copy begins three bytes in front of an aligned word (head bytes); margin 0:
    9 gw = 1 (mod 4): one byte behind the last whole word (a tail byte)."""
    p = dataclasses.replace(li.seam_case(gw)["params"], vertical_margin=margin)
    assert (p.grid_w, p.grid_h) == (gw, 9) and (margin * gw) % 4 == (gw % 4 if margin else 0) and (9 * gw) % 4 == 1
    return p


def seam_rows(gw):
    """(frame, [plane 0, plane 1], SEAM_HAND[gw]): the case's one frame under each of its two planes."""
    c = li.seam_case(gw)
    return case_frames(c)[0], [c["planes"][0], c["planes"][1]], list(li.SEAM_HAND[gw])


# ------------------------------------------------------------------ 5. 4K: both forms

@functools.lru_cache(maxsize=None)
def uhd_rows(vertical_mask):
    """(params, frames, plane, keep) of lanes_inputs.uhd_case: the same records and the (x 7 + y 13) & 0xFF plane; keep:
    30 % of the cells cleared at random."""
    c = li.uhd_case(vertical_mask)
    p = c["params"]
    keep = np.random.RandomState(4000).rand(p.grid_h, p.grid_w) >= 0.3
    return p, pd.freeze(case_frames(c)), c["planes"], frozen(keep)[0]


# ------------------------------------------------------------------ 6. a frame in three pieces

PIECES_CLEARED = [(li.PIECES_COLUMN, 0)]               # the cell of the records i % 6 == 0: 50 000 of the 300 000


@functools.lru_cache(maxsize=None)
def pieces_rows():
    """(params, frame, plane half, plane all, keep): one frame of lanes_inputs.pieces_case — 300 000 records, three pieces
    of the kernel's 131 072, all moving south-west into column 5, row i % 6.
      no mask   half: rows 3, 4, 5 vote: 3 centres; all: 6.  The word: present SW, dominant SW, count 300 000.
      keep clears (5, 0): its 50 000 records do not count: count 250 000.  half: 3 centres still (row 0 did not vote);
                all: rows 1 .. 5: 5."""
    c = li.pieces_case()
    p = c["params"]
    keep = np.ones((p.grid_h, p.grid_w), dtype=bool)
    for x, y in PIECES_CLEARED:
        keep[y, x] = False
    return p, case_frames(c)[0], c["planes"][0], c["planes"][1], frozen(keep)[0]


PIECES_HAND = {False: ([3, 6], word(1 << li.PIECES_SECTOR, li.PIECES_SECTOR, li.PIECES_N)),
               True: ([3, 5], word(1 << li.PIECES_SECTOR, li.PIECES_SECTOR, li.PIECES_N - li.PIECES_N // 6))}


# ------------------------------------------------------------------ 7. an empty analysed range

@functools.lru_cache(maxsize=None)
def empty_range_case():
    """(params, frames): 1080p with vertical_mask 0.5 — no analysed row (y_hi == y_lo) — and frames full of moving records:
    every flag and word reads 0, stored by the kernel's one exit (the frames have side data: the planner does not answer
    them)."""
    p = m.ScanParams.from_config(1920, 1080, vertical_mask=0.5)
    assert p.grid_h - 2 * p.vertical_margin <= 0
    rng = np.random.RandomState(50)
    q = m.ScanParams.from_config(1920, 1080)
    return p, pd.freeze([di.directed_frame(rng, q, 6) for _ in range(3)])


# ------------------------------------------------------------------ 8. stale results in a reused pinned block

def stale_case():
    """pipe_dir_inputs.stale_case() under a plane of 0xFF: by P3 the direction pipe's hand values under every sector."""
    return pd.stale_case()


# ------------------------------------------------------------------ 9. limits

def _accepts(preview, p):
    try:
        return preview(p)
    except m.MtgpuError as e:
        assert e.code == m._abi.MT_ERR_UNSUPPORTED
        return None


def _staged(p):
    r = _accepts(m.lanes_preview, p)
    return None if r is None else r["staged"]


@functools.lru_cache(maxsize=None)
def limit_shapes():
    """{"staged": the tallest 65-wide grid mtgpu_lanes_preview accepts staged, "unstaged": the first one it accepts only
    unstaged (one row more), "masked": the tallest one mtgpu_zones_preview accepts} as (gw, gh), found with the previews
    as derived_cliff_inputs finds its shapes."""
    staged = dc.largest(lambda gh: _staged(dc.grid_params(65, gh)) == 1)
    masked = dc.largest(lambda gh: _accepts(m.zones_preview, dc.grid_params(65, gh)) is not None)
    return {"staged": (65, staged), "unstaged": (65, staged + 1), "masked": (65, masked)}


limit_params = pd.limit_params
limit_frames = pd.limit_frames


def limit_plane(gw, gh):
    """The limit frames' pairs — (1, 0) / (2, 0) E, (gw - 3, gh - 1) / (gw - 2, gh - 1) W, (1, mid) / (2, mid) S — under a
    plane that holds E in the first row, W in the last one and 0xFF between them, except N alone in (2, mid).
    clusters_needed 2.  By hand, frame 0: the E pair votes (2 centres), the W pair votes (2), of the S pair only (1, mid)
    votes (alone: 0): 4 centres; frame 1 (the W pair alone): 2; frame 2 has no side data: 0.  Under the keep plane of
    limit_frames (it clears the S pair) the same centres; the word loses S."""
    plane = np.full((gh, gw), 0xFF, dtype=np.uint8)
    plane[0], plane[gh - 1] = 1 << E, 1 << W
    plane[gh // 2, 2] = 1 << N
    return frozen(plane)[0]


LIMIT_HAND = {False: ([4, 2, 0], [word(0x15, E, 2), word(0x10, W, 2), 0]),
              True: ([4, 2, 0], [word(0x11, E, 2), word(0x10, W, 2), 0])}

FINE_KW = pd.FINE_KW


# ------------------------------------------------------------------ 10. random draws

N_DRAWS = pd.N_DRAWS


@functools.lru_cache(maxsize=None)
def draw(i):
    """Draw i -> (params, frames, keep, chain): pipe_dir_inputs.draw(i)'s grid, frames and keep plane with
    lanes_inputs.draw's chain of five nested random planes on that grid (zeros, a & b, a, a | c, 0xFF: P6)."""
    p, frames, keep = pd.draw(i)
    rng = np.random.RandomState(9000 + i)
    a, b, c = (rng.randint(0, 256, size=(p.grid_h, p.grid_w)).astype(np.uint8) for _ in range(3))
    chain = [np.zeros_like(a), a & b, a, a | c, np.full_like(a, 0xFF)]
    frozen(*chain)
    return p, frames, keep, tuple(chain)


# ------------------------------------------------------------------ 11. a recording for mtgpu_scan_file and the host layer

REC_FRAMES, REC_FPS = 90, 25.0
REC_CFG = dict(mv_threshold_sq=4.0, vectors_needed=2, clusters_needed=1, vertical_mask=0.0)
REC_ENV = dict(MV_THRESHOLD_SQ="4", VECTORS_NEEDED="2", CLUSTERS_NEEDED="1", VERTICAL_MASK="0")
CLOCK = [(15, 9), (16, 9), (17, 9)]                    # a burnt-in clock in the last row
AGAINST = list(range(40, 50)) + list(range(60, 70))


@functools.lru_cache(maxsize=None)
def recording_case():
    """(params, frames[90], pts, keep, learned plane by hand): the two-way road of tests/test_gpu_lanes.py — 320 x 160
    pixels, 20 x 10 cells, 25 fps; frames 0 .. 29 one object goes WEST along row 2 and one EAST along row 7 (the learning
    stretch), frames 40 .. 49 one goes EAST along row 2, against its half, frames 60 .. 69 one WEST along row 7, against
    its half, frames 80 .. 89 both halves flow their usual way — with a clock burnt into cells (15 .. 17, 9): two records
    per cell in EVERY frame, moving towards sector f % 8.  Every sector holds an eighth of the clock's records, so
    `--learn --share 0.4` finds no usual sector there: the learned byte is 0x00, the inverted one 0xFF, and under the
    inverted plane the clock alone flags every frame.  keep clears the clock: the frames 40 .. 49 and 60 .. 69 remain.
    The learned plane by hand: 0x38 (W with NW, SW) in row 2 and 0x83 (E with NE, SE) in row 7, columns 2 .. 18; 0x00 in
    the clock's cells; 0xFF elsewhere."""
    def obj(col0, row, dx):
        return voters([(col0 + c, row, 2, dx, 0) for c in range(3)])
    frames = []
    for f in range(REC_FRAMES):
        d = di.DISP[f % 8]
        parts = [voters([(x, y, 2, d[0], d[1]) for x, y in CLOCK])]
        if f < 30:
            parts += [obj(2 + f // 2, 2, -6), obj(2 + f // 2, 7, 6)]
        elif 40 <= f < 50:
            parts += [obj(5 + (f - 40) // 2, 2, 6)]
        elif 60 <= f < 70:
            parts += [obj(5 + (f - 60) // 2, 7, -6)]
        elif f >= 80:
            parts += [obj(5 + (f - 80) // 2, 2, -6), obj(5 + (f - 80) // 2, 7, 6)]
        frames.append(m.FrameBatch.from_frames(parts).mv)
    p = m.ScanParams.from_config(320, 160, **REC_CFG)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (20, 10, 0)
    keep = np.ones((10, 20), dtype=bool)
    hand = np.full((10, 20), 0xFF, dtype=np.uint8)
    hand[2, 2:19], hand[7, 2:19] = 0x38, 0x83
    for x, y in CLOCK:
        keep[y, x] = False
        hand[y, x] = 0x00
    # pts as the front end forms them: ticks x time base (1 / 25)
    return p, pd.freeze(frames), tuple(f * (1.0 / REC_FPS) for f in range(REC_FRAMES)), frozen(keep)[0], frozen(hand)[0]


recording_stats = pd.recording_stats
