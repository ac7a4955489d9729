"""Inputs of tests/test_gpu_pipe_dir.py (the direction filter carried through the pipe, under its keep mask;
include/mtgpu_pipe_dir.h), built once and frozen, and the model.  The model states consequence D4 of the header literally
and adds nothing of its own:

    centres      remove every record of a forbidden sector (dir_model.passes) -> the masked plain pipe
                 (pipe_gmc_inputs.masked_plain: the zones model's AND rule; no keep plane: the plain scan)
    sector word  remove every record of a keep-0 cell -> the rose of tests/dir_model.py -> direction.sector_word

tests/test_pipe_dir_host.py checks, without a GPU, that the model returns every hand-derived number below and that it
agrees with the unchanged oracle through removal on every input.  Frames are lists; None is a frame without side data.

The hand frames live on the 6 x 5 grid of dir_inputs (SMALL_KW: 16-pixel cells, threshold 4, one vote makes a cell
active, one centre makes a flag, no margin); columns 1 .. 4 can be centres."""
import dataclasses
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import direction, synth

import derived_cliff_inputs as dc
import dir_inputs as di
import dir_model as dm
import oracle_binding as ob
import pipe_gmc_inputs as pg
from derived_edge_inputs import frozen, voters
from derived_soak import SHIFT_P

E, SE, S, SW, W, NW, N, NE = range(8)


# ------------------------------------------------------------------ the model

def remove_forbidden(frame, allow):
    """The frame without the records whose sector `allow` forbids (a record without a sector stays)."""
    return np.ascontiguousarray(frame[dm.passes(frame, allow)])


def remove_masked(p, frame, keep):
    """The frame without the records whose destination cell has keep bit 0."""
    return pg.remove_masked(p, frame, keep)


def sector_words(p, frames, keep=None):
    out = []
    for f in frames:
        if f is None:
            out.append(0)
            continue
        g = f if keep is None else remove_masked(p, f, keep)
        out.append(direction.sector_word(dm.frame_np(p, g, 0xFF)[1]))
    return out


def model(p, frames, allow, keep=None):
    """(flags, centres, sector words) lists of the direction pipe on `frames`."""
    fl, ce = pg.masked_plain(p, [None if f is None else remove_forbidden(f, allow) for f in frames], keep)
    return fl, ce, sector_words(p, frames, keep)


def oracle_centres(p, frames, allow, keep=None):
    """The same centres from the unchanged oracle, through removal: the forbidden records out and, under a keep plane,
    the records of keep-0 cells out as well — with vectors_needed >= 1 a cell without a vote is inactive, exactly as a
    cell whose keep bit is 0 (vectors_needed == 0 has no such removal: every cell is active without a vote)."""
    assert keep is None or p.vectors_needed >= 1
    parts = []
    for f in frames:
        g = np.zeros(0, dtype=m.MV_DTYPE) if f is None else remove_forbidden(f, allow)
        parts.append(g if keep is None else remove_masked(p, g, keep))
    b = m.FrameBatch.from_frames(parts)
    sd = np.array([f is not None for f in frames], dtype=np.uint8)
    return ob.scan_centres(p, b.mv, b.frame_off, sd, nthreads=4)[1].tolist()


def word(present, dominant, count):
    return present | (dominant << 8) | (count << 11)


def freeze(frames):
    for f in frames:
        if f is not None:
            f.setflags(write=False)
    return tuple(frames)


def case_frames(case):
    """A dir_inputs case -> its frames as a list (None: no side data)."""
    mv, off, sd = case["mv"], case["off"], case["sd"]
    return [np.array(mv[int(off[f]):int(off[f + 1])]) if sd[f] else None for f in range(len(off) - 1)]


def case_allows(case):
    """The allow byte of every frame of a dir_inputs case (every one of its frames belongs to a stream, or it has none)."""
    return dm.frame_allows(len(case["off"]) - 1, case["allow"], case["soff"], case["allows"]).tolist()


# ------------------------------------------------------------------ 1. the hand cases of dir_inputs through a pipe

BOUNDARY_WORD = word(0x07, E, 2)                       # rose 2 / 2 / 1: the tie goes to the smallest k


# ------------------------------------------------------------------ 2. hand frames under a mask

def small_params(**kw):
    p = m.ScanParams.from_config(96, 80, **dict(di.SMALL_KW, **kw))
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (6, 5, 0)
    return p


def small_keep(cleared):
    k = np.ones((5, 6), dtype=bool)
    for x, y in cleared:
        k[y, x] = False
    return frozen(k)[0]


@functools.lru_cache(maxsize=None)
def mask_hand():
    """{name: (params, frame, keep, allow, (centres, word) under the mask, (centres, word) without it)}.
    a  Row 1: two E records in each of (1, 1), (2, 1), (3, 1) — the keep plane clears the three cells; row 3: one W
       record in each of (1, 3), (2, 3), kept.  All sectors allowed.
       Mask: the six E records do not count: present = W only, dominant W, count 2; active (1, 3), (2, 3), neighbours:
       2 centres.  No mask: n[E] = 6, n[W] = 2: present E | W, dominant E, count 6; row 1 gives 3 centres: 5.
       A build whose mask reaches only the active plane reports 2 centres and the word of 6 E records.
    b  vectors_needed == 0, the boundary frame, keep clears (2, 2): active = keep.  20 candidate cells (5 rows x columns
       1 .. 4) less the cleared one, every other one has an active neighbour: 19.  No record lies in (2, 2): the word is
       that of rose 2 / 2 / 1.  No mask: 20.
    b0 the same with a frame that has side data and no record: 19 and word 0; no mask: 20.
    c  Row 2: (0, 2) E, (1, 2) E | (2, 2) E, cleared | (3, 2) W, (4, 2) W.  allow = E.
       Mask: active (0, 2), (1, 2); (1, 2) has a neighbour and lies in columns 1 .. 4: 1 centre.  n[E] = 2 (the record of
       the cleared cell does not count), n[W] = 2: present E | W, the tie goes to E, count 2.
       No mask: active (0, 2), (1, 2), (2, 2): centres (1, 2), (2, 2): 2; n[E] = 3: dominant E, count 3.
    c-all  the same under every sector.  Mask: active 0, 1, 3, 4: centres (1, 2), (3, 2), (4, 2): 3.  No mask: 4."""
    a = voters([(1, 1, 2, 5, 0), (2, 1, 2, 5, 0), (3, 1, 2, 5, 0), (1, 3, 1, -5, 0), (2, 3, 1, -5, 0)])
    b = voters(di.BOUNDARY_CELLS)
    c = voters([(0, 2, 1, 5, 0), (1, 2, 1, 5, 0), (2, 2, 1, 5, 0), (3, 2, 1, -5, 0), (4, 2, 1, -5, 0)])
    rng = np.random.RandomState(21)
    a, c = a[rng.permutation(len(a))], c[rng.permutation(len(c))]
    p1, p0 = small_params(), small_params(vectors_needed=0)
    ka, kb = small_keep([(1, 1), (2, 1), (3, 1)]), small_keep([(2, 2)])
    out = {
        "a": (p1, a, ka, 0xFF, (2, word(0x10, W, 2)), (5, word(0x11, E, 6))),
        "b": (p0, b, kb, 0x04, (19, BOUNDARY_WORD), (20, BOUNDARY_WORD)),
        "b0": (p0, b[:0], kb, 0xFF, (19, 0), (20, 0)),
        "c": (p1, c, kb, 0x01, (1, word(0x11, E, 2)), (2, word(0x11, E, 3))),
        "c-all": (p1, c, kb, 0xFF, (3, word(0x11, E, 2)), (4, word(0x11, E, 3))),
    }
    for v in out.values():
        v[1].setflags(write=False)
    return out


# ------------------------------------------------------------------ 3. D1 - D4: every layout and batch geometry

SHAPE_ALLOWS = [0xFF, 0x5B, 0x01]


@functools.lru_cache(maxsize=None)
def shapes_case():
    """(params, frames[14], keep) on the 80 x 6 grid, vectors_needed 2: frames without side data first, interleaved and
    last; a frame with side data and no record; blobs whose records move in every direction; one frame of 4 097 records
    (several trips of the streamers) and one of a single record.  keep: 25 % of the cells cleared at random."""
    p = m.ScanParams.from_config(1280, 96, **dict(di.SMALL_KW, vectors_needed=2))
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (80, 6, 0)
    rng = np.random.RandomState(2100)
    d = [di.directed_frame(rng, p, 6 + i) for i in range(8)]
    frames = [None, d[0], d[1], None, d[2], np.zeros(0, dtype=m.MV_DTYPE), d[3], np.array(di.edge_frame(4097)), None, d[4], d[5],
              d[6], d[7][:1].copy(), None]
    keep = rng.rand(p.grid_h, p.grid_w) >= 0.25
    return p, freeze(frames), frozen(keep)[0]


# ------------------------------------------------------------------ 4. the streamers' edges

# The seams of dir_inputs.seam_case under a keep plane that clears the cell on each side of a seam in row 1: (63, 1) and
# (64, 1), and on the 129-wide grid (127, 1) and (128, 1) too.  SEAM_HAND less what row 1 gave:
#   65   all  row 1 gave 1 (63): 5 - 1 = 4.   E  row 1 gave 1 (63, its neighbour 64): 2 - 1 = 1.   W  0.
#   129  all  row 1 gave 2 at 63 | 64 and 2 at 126, 127 (126 W is now alone): 12 - 4 = 8.
#        E    row 1 gave 2 at 63 | 64 and 1 at 127: 5 - 3 = 2.   W  0.
SEAM_CLEARED = {65: [(63, 1), (64, 1)], 129: [(63, 1), (64, 1), (127, 1), (128, 1)]}
SEAM_MASKED_HAND = {65: [4, 1, 0], 129: [8, 2, 0]}


def seam_keep(gw):
    k = np.ones((9, gw), dtype=bool)
    for x, y in SEAM_CLEARED[gw]:
        k[y, x] = False
    return frozen(k)[0]


BIG_N, BIG_SECTOR = 262145, SW                         # three pieces of kDirChunk = 131 072 records


@functools.lru_cache(maxsize=None)
def big_case():
    """(params, frame): 262 145 records on the 80 x 6 grid; sector 3 gets the bulk, each other sector one record, spread
    through the three pieces.  The word: present 0xFF, dominant 3, count 262 138."""
    p = m.ScanParams.from_config(1280, 96, **dict(di.SMALL_KW, vectors_needed=3))
    i = np.arange(BIG_N, dtype=np.int64)
    sec = np.full(BIG_N, BIG_SECTOR, dtype=np.int64)
    others = [s for s in range(8) if s != BIG_SECTOR]
    sec[[5 + 40000 * j for j in range(7)]] = others
    d = np.array(di.DISP, dtype=np.int64)[sec]
    mv = np.zeros(BIG_N, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"] = (i % 80) * 16 + 8, ((i // 80) % 6) * 16 + 8
    mv["src_x"], mv["src_y"] = mv["dst_x"] - d[:, 0], mv["dst_y"] - d[:, 1]
    return p, frozen(mv)[0]


BIG_WORD = word(0xFF, BIG_SECTOR, BIG_N - 7)


# ------------------------------------------------------------------ 5. stale results in a reused pinned block

@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, batch 1, batch 2, hand 1, hand 2) on the 6 x 5 grid under every sector, no mask.
    Batch 1: three boundary frames: flag 1, 5 centres, the word of rose 2 / 2 / 1 in every slot.
    Batch 2, into the same slots: frame c of mask_hand() (flag 1, 4 centres, n[E] = 3 and n[W] = 2: present E | W,
    dominant E, count 3); one E record alone in (1, 1) (flag 0, 0 centres, the word of one E record: the kernel's store
    of a frame that ends without a centre); no side data (0, 0, 0: the planning kernel's store)."""
    one = [np.array(voters(di.BOUNDARY_CELLS)) for _ in range(3)]
    two = [np.array(mask_hand()["c"][1]), voters([(1, 1, 1, 5, 0)]), None]
    h1 = {"flags": [1, 1, 1], "centres": [5, 5, 5], "sectors": [BOUNDARY_WORD] * 3}
    h2 = {"flags": [1, 0, 0], "centres": [4, 0, 0], "sectors": [word(0x11, E, 3), word(0x01, E, 1), 0]}
    return small_params(), freeze(one), freeze(two), h1, h2


# ------------------------------------------------------------------ 6. limits

FINE_KW = pg.FINE_KW


def _accepts(preview, p):
    try:
        preview(p)
        return True
    except m.MtgpuError as e:
        assert e.code == m._abi.MT_ERR_UNSUPPORTED
        return False


@functools.lru_cache(maxsize=None)
def limit_shape():
    """(gw, gh) of the tallest 65-wide grid mtgpu_dir_preview accepts, found with the preview as derived_cliff_inputs
    finds its shapes."""
    return 65, dc.largest(lambda gh: _accepts(m.dir_preview, dc.grid_params(65, gh)))


@functools.lru_cache(maxsize=None)
def masked_limit_shape():
    """(gw, gh) of the tallest 65-wide grid mtgpu_zones_preview accepts."""
    return 65, dc.largest(lambda gh: _accepts(m.zones_preview, dc.grid_params(65, gh)))


def limit_params(gw, gh):
    return dc.grid_params(gw, gh, vectors_needed=1, mv_threshold_sq=16.0, clusters_needed=2)


def limit_frames(gw, gh):
    """(frames, keep): pairs at the corners of the grid.  First row: (1, 0) E, (2, 0) E; the far corner of the last row:
    (gw - 3, gh - 1) W, (gw - 2, gh - 1) W; the middle row: (1, mid) S, (2, mid) S, which `keep` clears.  A second frame
    holds only the far corner's pair; then no side data."""
    sh = dc.shift_of(gw, gh)
    mid = gh // 2
    far = [(gw - 3, gh - 1, 1, -5, 0), (gw - 2, gh - 1, 1, -5, 0)]
    one = voters([(1, 0, 1, 5, 0), (2, 0, 1, 5, 0)] + far + [(1, mid, 1, 0, 5), (2, mid, 1, 0, 5)], sh)
    keep = np.ones((gh, gw), dtype=bool)
    keep[mid, 1] = keep[mid, 2] = False
    return freeze([one, voters(far, sh), None]), frozen(keep)[0]


# by hand, clusters_needed 2: every pair gives 2 centres
#   no mask   all: 6, 2;  E | S: 4, 0;  W: 2, 2        words: E 2, S 2, W 2 -> present 0x15, dominant E, count 2; W 2
#   mask      all: 4, 2;  E | S: 2, 0;  W: 2, 2        words: E 2, W 2 -> present 0x11, dominant E, count 2; W 2
LIMIT_ALLOWS = [0xFF, 0x05, 0x10]
LIMIT_HAND = {False: ([[6, 2, 0], [4, 0, 0], [2, 2, 0]], [word(0x15, E, 2), word(0x10, W, 2), 0]),
              True: ([[4, 2, 0], [2, 0, 0], [2, 2, 0]], [word(0x11, E, 2), word(0x10, W, 2), 0])}


# ------------------------------------------------------------------ 8. random draws

N_DRAWS = 40
DRAW_ALLOWS = di.DRAW_ALLOWS


@functools.lru_cache(maxsize=None)
def draw(i):
    """Draw i of N_DRAWS -> (params, frames, keep): as dir_inputs.draw — block_shift 1 .. 5 with the soak's weights,
    vectors_needed i % 4, a margin of (i // 4) % 4 rows where the grid has more than twice as many, up to 12 frames of up
    to 2 700 random records plus at most 291 of blobs whose records move in every direction — but on a grid that BOTH
    mtgpu_dir_preview and mtgpu_zones_preview accept (w in [64, 2000), h in [64, 1200): every such grid passes the masked
    scan's limit, so no draw is skipped), and with a drawn keep plane: a share of 5 %, 30 % or 70 % of the cells cleared."""
    rng = np.random.RandomState(9100 + i)
    while True:
        sh = int(rng.choice([1, 2, 3, 4, 5], p=SHIFT_P))
        w, h = int(rng.randint(64, 2000)), int(rng.randint(64, 1200))
        p = m.ScanParams.from_config(w, h, mv_threshold_sq=float(rng.choice([16.0, 4.0, 0.0, 9.5])), block_size=1 << sh, block_shift=sh,
                                     vectors_needed=i % 4, clusters_needed=int(rng.choice([1, 2, 3])), vertical_mask=0.0)
        margin = (i // 4) % 4
        if 2 * margin >= p.grid_h:
            margin = 0
        p = dataclasses.replace(p, vertical_margin=margin)
        try:
            m.plan_preview(p)
            m.dir_preview(p)
            m.zones_preview(p)
            break
        except m.MtgpuError:
            continue
    F = int(rng.randint(1, 13))
    mv, off, _ = synth.random_frames(rng, F, 2700, w, h, hot=float(rng.choice([0.05, 0.5, 0.95])))
    frames = []
    for f in range(F):
        # (from_frames lays the two parts out as 40-byte records: np.concatenate alone would pack them into 32 bytes)
        part = m.FrameBatch.from_frames([mv[int(off[f]):int(off[f + 1])], di.directed_frame(rng, p, 4 + 4 * (f % 3))]).mv
        assert part.dtype == m.MV_DTYPE and part.dtype.itemsize == 40
        frames.append(part[rng.permutation(len(part))] if f == 0 or rng.rand() < 0.85 else None)
    keep = rng.rand(p.grid_h, p.grid_w) >= float(rng.choice([0.05, 0.3, 0.7]))
    return p, freeze(frames), frozen(keep)[0]


# ------------------------------------------------------------------ 9. a recording for mtgpu_scan_file and the host layer

REC_FRAMES, REC_FPS = 40, 25.0
EAST, WEST = range(5, 15), range(24, 30)
CLOCK = pg.block(5, 6, 4, 2)                           # a burnt-in clock: its blocks flicker downwards in every frame
OBJECT = pg.block(50, 30, 3, 2)


@functools.lru_cache(maxsize=None)
def recording_case():
    """(params, frames[40], pts, keep) at the 1080p defaults (120 x 68 cells, rows 3 .. 64 analysed, threshold 16, two
    votes make a cell active, two centres a flag).  Every frame with side data carries the clock, eight cells whose
    records move by (0, 5): alone it flags every frame, under any byte that allows S.  Frames 5 .. 14 also carry a 3 x 2
    object moving east by (6, 0), frames 24 .. 29 one moving west by (-6, 0).  Frames 0 and 20 have no side data.  keep
    clears the clock.  Under the mask: --ignore W,NW,SW keeps frames 5 .. 14, --ignore E,NE,SE keeps 24 .. 29."""
    frames = []
    for f in range(REC_FRAMES):
        if f in (0, 20):
            frames.append(None)
            continue
        groups = [(CLOCK, (0, 5))]
        if f in EAST:
            groups.append((OBJECT, (6, 0)))
        if f in WEST:
            groups.append((OBJECT, (-6, 0)))
        frames.append(pg.cells_frame(groups))
    # pts as the front end forms them: ticks x time base (1 / 25)
    return pg.params(), freeze(frames), tuple(f * (1.0 / REC_FPS) for f in range(REC_FRAMES)), pg.keep_without(CLOCK)


def recording_stats(words):
    """(frames, present[8], dominant[8]) of a list of sector words, as mtgpu_scan_file --dir-sectors prints them."""
    present, dominant, frames = [0] * 8, [0] * 8, 0
    for w in words:
        pr, dom, _ = direction.unpack_sector_word(w)
        if w:
            frames += 1
            dominant[dom] += 1
            for k in range(8):
                present[k] += (pr >> k) & 1
    return frames, present, dominant
