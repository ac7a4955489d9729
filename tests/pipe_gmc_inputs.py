"""Inputs of tests/test_gpu_pipe_gmc.py (global-motion compensation carried through the pipe, under its keep mask;
include/mtgpu_pipe_gmc.h), built once and frozen, and the model: tests/gmc_model.py and the zones model's AND rule, with
the one thing the header adds — the MASKED ESTIMATE: a record is counted iff it passes the bounds test of :262 and the
keep bit of its destination cell is set.  Every expected value is either derived by hand in the docstring of its case or
comes from the model; tests/test_pipe_gmc_host.py checks, without a GPU, that the model returns every hand-derived number
below and that P2 - P4 of the header hold inside it.

The hand frames live on the 1080p default grid: 120 x 68 cells of 16 pixels, VERTICAL_MASK 0.05 (rows 3 .. 64 are
analysed), MV_THRESHOLD_SQ 16, VECTORS_NEEDED 2, CLUSTERS_NEEDED 2.  The camera's pan is (9, 3): 81 + 9 = 90 >= 16, so
a panned record passes the plain threshold, and a still record's residual under the pan, (-9, -3), passes as well."""
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import synth

import gmc_model as gm
import zones_inputs as zi
from derived_edge_inputs import frozen, voters

GW, GH, MARGIN, VN, CN, THR = 120, 68, 3, 2, 2, 16.0
PAN = (9, 3)
MS, Q8 = 16, 128


def params(**kw):
    p = m.ScanParams.from_config(1920, 1080, **kw)
    if not kw:
        assert (p.grid_w, p.grid_h, p.vertical_margin, p.vectors_needed, p.clusters_needed, p.mv_threshold_sq, p.block_shift) == \
            (GW, GH, MARGIN, VN, CN, THR, 4)
    return p


def block(x0, y0, w, h):
    return [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]


def cells_frame(groups):
    """groups = [(cells, (dx, dy))]: VECTORS_NEEDED records per cell, dst - src = (dx, dy)."""
    return voters([(x, y, VN, d[0], d[1]) for cells, d in groups for x, y in cells], 4)


def keep_without(cells):
    k = np.ones((GH, GW), dtype=bool)
    for x, y in cells:
        k[y, x] = False
    return frozen(k)[0]


def pack_vector(gx, gy):
    """(uint16)gx | (uint16)gy << 16: what MT_PIPE_REPORT_VECTOR stores."""
    return (int(gx) & 0xFFFF) | ((int(gy) & 0xFFFF) << 16)


def unpack_vector(w):
    gx, gy = int(w) & 0xFFFF, (int(w) >> 16) & 0xFFFF
    return (gx - 65536 if gx >= 32768 else gx), (gy - 65536 if gy >= 32768 else gy)


# ------------------------------------------------------------------ the model

def counted(p, mv, keep=None):
    """Step 1 on the decode path: the bounds test of :262 AND, with a keep plane, the keep bit of the destination cell."""
    inside = gm.counted(p, mv)
    if keep is None:
        return inside
    cx, cy = gm.cells(p, mv)
    bit = np.asarray(keep, dtype=bool)[np.clip(cy, 0, p.grid_h - 1), np.clip(cx, 0, p.grid_w - 1)]
    return inside & bit


def estimate(p, mv, max_shift, min_share_q8, keep=None):
    """Steps 1 - 4 over the counted records only -> (gx, gy, n_in, mode_x, n_x, mode_y, n_y)."""
    inside = counted(p, mv, keep)
    n_in = int(inside.sum())
    dx, dy = gm.displacements(mv)
    mx, nx = gm.mode_of(dx[inside], max_shift)
    my, ny = gm.mode_of(dy[inside], max_shift)
    gx = mx if nx * 256 >= min_share_q8 * n_in else 0
    gy = my if ny * 256 >= min_share_q8 * n_in else 0
    return gx, gy, n_in, mx, nx, my, ny


def residual_centres(p, mv, gx, gy, keep=None):
    """Step 5: EVERY record inside the bounds votes its residual; active = votes >= vn AND (keep OR the row is not
    analysed) — the masked plane of mtgpu_zones.h; centres as the scan's."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    votes = np.zeros((gh, gw), dtype=np.int64)
    t = gm.threshold_int(p.mv_threshold_sq)
    if len(mv) and t is not None:
        dx, dy = gm.displacements(mv)
        rx, ry = dx - gx, dy - gy
        cx, cy = gm.cells(p, mv)
        ok = gm.counted(p, mv) & (rx * rx + ry * ry >= t)
        np.add.at(votes, (cy[ok], cx[ok]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    if keep is not None:
        act = act & (np.asarray(keep, dtype=bool) | ~rows)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    return int((act & nb & rows)[:, 1:gw - 1].sum())


def model(p, frames, max_shift, min_share_q8, keep=None):
    """(flags, centres, packed vectors) lists of the compensated pipe on `frames` (None: no side data -> 0, 0, 0)."""
    fl, ce, ve = [], [], []
    for f in frames:
        if f is None:
            fl.append(0), ce.append(0), ve.append(0)
            continue
        gx, gy = estimate(p, f, max_shift, min_share_q8, keep)[:2]
        c = residual_centres(p, f, gx, gy, keep)
        fl.append(int(c >= max(1, p.clusters_needed))), ce.append(c), ve.append(pack_vector(gx, gy))
    return fl, ce, ve


def masked_plain(p, frames, keep=None):
    """(flags, centres) of the pipe WITHOUT compensation under `keep` (the zones model's AND rule; None: the plain scan)."""
    k = np.ones((p.grid_h, p.grid_w), dtype=bool) if keep is None else keep
    ce = [0 if f is None else zi.zone_counts_np(p, f, k)[0] for f in frames]
    return [int(c >= max(1, p.clusters_needed)) for c in ce], ce


def remove_masked(p, frame, keep):
    """The frame with the records in keep-0 cells (of the grid) removed: P4's estimate input."""
    cx, cy = gm.cells(p, frame)
    inside = (cx >= 0) & (cx < p.grid_w) & (cy >= 0) & (cy < p.grid_h)
    bit = np.asarray(keep, dtype=bool)[np.clip(cy, 0, p.grid_h - 1), np.clip(cx, 0, p.grid_w - 1)]
    return np.ascontiguousarray(frame[~inside | bit])


def shifted(frame, gx, gy):
    """The frame with (gx, gy) added to every record's src, or None where an int16 would overflow."""
    return gm.shift_src(frame, np.array([0, len(frame)], dtype=np.uint64), [gx], [gy])


def freeze(frames):
    for f in frames:
        if f is not None:
            f.setflags(write=False)
    return tuple(frames)


# ------------------------------------------------------------------ 1. the hand frames

PAN_ROWS = block(0, 20, GW, 20)                    # rows 20 .. 39, every column: 2400 cells, 4800 records
OBJECT = block(50, 25, 2, 2)                       # inside the pan rows; moves by (14, 3): residual (5, 0), 25 >= 16
OVERLAY_C = block(5, 6, 10, 3)                     # 30 cells, 60 still records: fewer than the pan's 4800
PAN_SMALL = block(30, 20, 20, 2)                   # 40 cells, 80 records
OVERLAY_D = block(5, 6, 20, 4)                     # 80 cells, 160 still records: more than PAN_SMALL's 80
E_PAN = [(30, 20), (31, 20)]                       # 4 records at (9, 3)
E_OTHER = [(40, 30), (41, 30)]                     # 4 records, four other displacements
E_OTHER_D = [(5, -5), (6, -6), (7, -7), (8, -8)]
E_STILL = block(60, 40, 4, 1)                      # 8 still records


@functools.lru_cache(maxsize=None)
def hand_frames():
    """{name: frame}.
    a  the pan on rows 20 .. 39.  Plain: every cell of the 20 rows is active, columns 1 .. 118 are centres: 20 * 118 =
       2360, flag 1.  Compensated: mode (9, 3) with all 4800 counted records, every residual 0: centres 0, flag 0.
    b  the same, but the 2 x 2 object moves by (14, 3).  Mode (9, 3) with 4792 of 4800 on x, all on y; the object's
       residual (5, 0) passes, its four cells are neighbours: centres 4, flag 1.
    c  a plus the overlay of 30 still cells on rows 6 .. 8.  n_in 4860, mode (9, 3) with 4800: 4800 * 256 >= 128 * 4860.
       The overlay's residual (-9, -3) passes: 30 centres (columns 5 .. 14, every cell has a neighbour), flag 1.  Under a
       keep plane clearing the overlay: n_in 4800, the same vector, the overlay's cells are not active: 0, flag 0.
    d  the small pan (80 records) and the large overlay (160 still records).  No mask: n_in 240, mode 0 with 160 on both
       axes, nothing is compensated; the overlay's residual is 0, the pan's cells are active: 2 rows x 20 columns = 40
       centres, flag 1.  Keep clearing the overlay: n_in 80, mode (9, 3) with 80: the vector reads (9, 3), centres 0, flag 0.
    e  4 pan records, 4 records at (5, -5), (6, -6), (7, -7), (8, -8), 8 still records in four cells, min_share_q8 128.
       Keep clearing the still cells: n_in 8, mode (9, 3) with 4: 4 * 256 = 1024 >= 128 * 8 = 1024, applied.  The pan's
       cells go quiet; the four others keep residuals (-4, -8) .. (-1, -11), all >= 16, two per cell, the two cells are
       neighbours: centres 2, flag 1 (the still cells would pass, (-9, -3), but their keep bit is 0).  All-ones keep (or
       none): n_in 16, mode 0 with 8 on both axes (8 * 256 >= 128 * 16: supported, and 0), the pan's 4 * 256 < 128 * 16
       would not be; nothing is subtracted: the pan's two cells and the others' two cells are active: centres 4, flag 1."""
    e_cells = [(x, y, VN) + PAN for x, y in E_PAN] + [(E_OTHER[i // 2][0], E_OTHER[i // 2][1], 1) + E_OTHER_D[i] for i in range(4)] + \
        [(x, y, VN, 0, 0) for x, y in E_STILL]
    fr = {
        "a": cells_frame([(PAN_ROWS, PAN)]),
        "b": cells_frame([([c for c in PAN_ROWS if c not in OBJECT], PAN), (OBJECT, (14, 3))]),
        "c": cells_frame([(PAN_ROWS, PAN), (OVERLAY_C, (0, 0))]),
        "d": cells_frame([(PAN_SMALL, PAN), (OVERLAY_D, (0, 0))]),
        "e": voters(e_cells, 4),
    }
    rng = np.random.RandomState(12)
    for k in fr:
        fr[k] = fr[k][rng.permutation(len(fr[k]))]
        assert fr[k].dtype == m.MV_DTYPE and fr[k].dtype.itemsize == 40
        fr[k].setflags(write=False)
    return fr


KEEP_C, KEEP_D, KEEP_E = keep_without(OVERLAY_C), keep_without(OVERLAY_D), keep_without(E_STILL)
ONES = frozen(np.ones((GH, GW), dtype=bool))[0]

# name -> (frame, keep or None, "plain" | "gmc", (flag, centres, vector or None))   vector: only where compensated
HAND = [
    ("a-plain", "a", None, "plain", (1, 2360, None)),
    ("a-gmc", "a", None, "gmc", (0, 0, (9, 3))),
    ("b-gmc", "b", None, "gmc", (1, 4, (9, 3))),
    ("c-gmc-no-mask", "c", None, "gmc", (1, 30, (9, 3))),
    ("c-gmc-mask", "c", "C", "gmc", (0, 0, (9, 3))),
    ("d-plain", "d", None, "plain", (1, 40, None)),
    ("d-gmc-no-mask", "d", None, "gmc", (1, 40, (0, 0))),
    ("d-gmc-mask", "d", "D", "gmc", (0, 0, (9, 3))),
    ("e-gmc-mask", "e", "E", "gmc", (1, 2, (9, 3))),
    ("e-gmc-ones", "e", "ONES", "gmc", (1, 4, (0, 0))),
    ("e-gmc-no-mask", "e", None, "gmc", (1, 4, (0, 0))),
]
KEEPS = {"C": KEEP_C, "D": KEEP_D, "E": KEEP_E, "ONES": ONES, None: None}


# ------------------------------------------------------------------ 2. P1 - P4: every layout and batch shape

SHAKE = 5
SETTINGS = [(16, 128), (16, 64), (0, 128), (3, 0)]        # the default; a share the noisy synthetic background meets; P3; modes beyond max_shift


@functools.lru_cache(maxsize=None)
def shapes_case():
    """(params, frames[14], keep): frames without side data first, interleaved and last; a frame with side data and no
    record; three frames of synth.StreamSpec(shake=5) with an event (32 640 records each: many trips of the streamers);
    the five hand frames.  keep: the overlays of c, d and e cleared, and 25 % of the grid's cells cleared at random
    (so the shaking frames lose counted records and active cells)."""
    spec = synth.StreamSpec(shake=SHAKE, seed=3)
    spec.events = [synth.Event(1, 4, 400, 200, 6, 4, 9, 1)]
    sy = [synth.gen_frame(spec, i) for i in range(4)]
    assert sy[0] is None and all(f is not None for f in sy[1:])
    h = hand_frames()
    frames = [None, np.array(sy[1]), np.array(h["a"]), None, np.array(h["c"]), np.zeros(0, dtype=m.MV_DTYPE), np.array(sy[2]),
              np.array(h["d"]), None, np.array(h["b"]), np.array(h["e"]), np.array(sy[3]), np.array(h["e"][:1]), None]
    keep = np.random.RandomState(5).rand(GH, GW) >= 0.25
    for cells in (OVERLAY_C, OVERLAY_D, E_STILL):
        for x, y in cells:
            keep[y, x] = False
    return params(), freeze(frames), frozen(keep)[0]


# ------------------------------------------------------------------ 3. stale results in a reused pinned block

@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, batch 1, batch 2, hand 1, hand 2) at (16, 128), no mask.
    Batch 1: three frames c: flag 1, centres 30, vector (9, 3) in every slot.
    Batch 2, into the same slots: frame d (flag 1, centres 40, vector (0, 0)), frame a (flag 0, centres 0, vector (9, 3):
    the kernel's store of a frame that ends without a centre), no side data (0, 0, 0: the planning kernel's store)."""
    h = hand_frames()
    one = [np.array(h["c"]) for _ in range(3)]
    two = [np.array(h["d"]), np.array(h["a"]), None]
    h1 = {"flags": [1, 1, 1], "centres": [30, 30, 30], "vector": [pack_vector(9, 3)] * 3}
    h2 = {"flags": [1, 0, 0], "centres": [40, 0, 0], "vector": [0, pack_vector(9, 3), 0]}
    return params(), freeze(one), freeze(two), h1, h2


# ------------------------------------------------------------------ 4. limits

FINE_KW = dict(block_size=4, block_shift=2, vectors_needed=1)      # 3840 x 2160 -> 960 x 540 cells: row-banded, no gmc form


def limit_frames(gw, gh, sh, keep_clear):
    """Three frames on a gw x gh grid of (1 << sh)-pixel cells, vertical_mask 0, for GMC_PAN_KW-like settings
    (vectors_needed 1 here): a pan (7, -3) on the first, a middle and the last row; the same with an object pair at the
    far corner of the grid (last row, columns gw - 3 / gw - 2) moving by (12, -3); the same with a still overlay pair on
    the middle row (columns 1 / 2) that `keep_clear` names."""
    rows = sorted({0, gh // 2, gh - 1})
    pan = [(x, y, 1, 7, -3) for y in rows for x in range(gw)]
    obj = {(gw - 3, gh - 1), (gw - 2, gh - 1)}
    with_obj = [(x, y, 1, 12 if (x, y) in obj else 7, -3) for x, y, _, _, _ in pan]
    still = {c for c in keep_clear}
    with_still = [(x, y, 1, 0 if (x, y) in still else 7, 0 if (x, y) in still else -3) for x, y, _, _, _ in pan]
    return [voters(pan, sh), voters(with_obj, sh), voters(with_still, sh), None]


REC_FRAMES, REC_FPS = 40, 25.0


@functools.lru_cache(maxsize=None)
def recording_case():
    """(params, frames[40], pts, keep): a shaking camera with a burnt-in overlay, at the defaults.  Every frame with side
    data carries a pan on rows 20 .. 23 (480 cells) that changes from frame to frame, (1 + f % 7, -(f % 5)), and the
    overlay OVERLAY_C (still).  Frames 10 .. 19 also carry the 2 x 2 object, moving 6 pixels faster than the pan on x.
    Frame 0 and frame 20 have no side data.
    Plain: every frame with side data whose pan passes 16 is kept.  --gmc: the overlay keeps EVERY frame with a non-zero
    pan flagged (its residual is minus the pan).  --gmc --keep (the overlay cleared): only frames 10 .. 19 remain."""
    rows = block(0, 20, GW, 4)
    frames = []
    for f in range(REC_FRAMES):
        if f in (0, 20):
            frames.append(None)
            continue
        pan = (1 + f % 7, -(f % 5))
        groups = [([c for c in rows if not (10 <= f < 20 and c in block(50, 21, 2, 2))], pan), (OVERLAY_C, (0, 0))]
        if 10 <= f < 20:
            groups.append((block(50, 21, 2, 2), (pan[0] + 6, pan[1])))
        frames.append(cells_frame(groups))
    return params(), freeze(frames), tuple(float(f) / REC_FPS for f in range(REC_FRAMES)), KEEP_C
