"""numpy restatement of the heading scan (include/mtgpu_headings.h), composed from the existing models: the centre plane
and the flood fill of blobs_model, the order of objects_model.ranked, the counting records and the displacement of
dir_model, the sector of mvtrim_amd.direction.  tests/test_headings_host.py holds it to the hand numbers of
tests/headings_inputs.py and, through the unchanged oracle and dir_model, to consequences D and E."""
import numpy as np

import mvtrim_amd as m
from mvtrim_amd import direction

import blobs_model as bm
import dir_model as dm
import objects_model as om
import zones_inputs as zi

HEADING_DTYPE = m._abi.HEADING_DTYPE
NONE = 0xFFFFFFFF
K_MAX = om.K_MAX


def empty_motion(shape):
    mo = np.zeros(shape, dtype=HEADING_DTYPE)
    mo["heading"] = NONE
    return mo


def rank_plane(cen, k):
    """int [gh, gw]: the rank of the blob of every centre cell in the order of objects_model.ranked, -1 for a cell that is
    no centre or whose blob has rank k or beyond."""
    lab = bm.label(cen)
    n = int(lab.max())
    gw = cen.shape[1]
    blobs = []
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        blobs.append((-len(xs), int((ys * gw + xs).min()), i))
    rank_of = np.full(n + 1, -1, dtype=np.int64)
    for r, (_, _, i) in enumerate(sorted(blobs)[:k]):
        rank_of[i] = r
    return rank_of[lab]


def heading_of(n):
    """The sector with the largest count, the lowest on a tie; NONE when every count is 0."""
    n = [int(v) for v in n]
    return n.index(max(n)) if max(n) > 0 else NONE


def frame_motion(p, mv, cen, k):
    """HEADING_DTYPE [k] of one frame with side data: cen is its centre plane (bool [gh, gw])."""
    mo = empty_motion(k)
    ranks = rank_plane(cen, k)
    ok = dm.counting(p, mv)
    part = mv[ok]
    gx, gy = part["dst_x"].astype(np.int64) >> p.block_shift, part["dst_y"].astype(np.int64) >> p.block_shift
    r = ranks[gy, gx]                                    # counting: inside the grid
    dx, dy = dm.displacement(part)
    sec = direction.sector_of(dx, dy)
    for j in range(k):
        mine = r == j
        if not mine.any():
            continue
        n = np.bincount(sec[mine & (sec >= 0)], minlength=8)
        mo["n"][j], mo["records"][j], mo["heading"][j] = n, int(mine.sum()), heading_of(n)
        mo["sum_dx"][j], mo["sum_dy"][j] = int(dx[mine].sum()), int(dy[mine].sum())
    return mo


def allowed_np(lst, motion, min_blob_cells, allow):
    """uint32 [F]: the listed entries of at least min_blob_cells cells whose heading is NONE or allowed."""
    h = motion["heading"].astype(np.int64)
    ok = (h == NONE) | (((int(allow) >> np.minimum(h, 7)) & 1) != 0)
    return ((lst["cells"] >= max(1, min_blob_cells)) & ok).sum(axis=1).astype(np.uint32)


def flags_np(p, centres, allowed, min_objects):
    return ((np.asarray(centres) >= max(1, p.clusters_needed)) & (np.asarray(allowed) >= max(1, min_objects))).astype(np.uint8)


def model_batch(p, mv, off, sd, k=K_MAX, min_blob_cells=1, allow=0xFF, soff=None, keeps=None):
    """objects_model.model_batch's dict plus "motion": HEADING_DTYPE [F, k] and "allowed": uint32 [F]."""
    out = om.model_batch(p, mv, off, sd, k, min_blob_cells, soff, keeps)
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else np.zeros(F, dtype=np.int64)
    out["motion"] = empty_motion((F, k))
    for f in range(F):
        if not has[f] or (keeps is not None and not 0 <= st[f] < len(keeps)) or out["blobs"][f] == 0:
            continue
        part = mv[int(off[f]):int(off[f + 1])]
        cen = bm.centre_plane(p, part, None if keeps is None else keeps[st[f]])
        out["motion"][f] = frame_motion(p, part, cen, k)
    out["allowed"] = allowed_np(out["list"], out["motion"], min_blob_cells, allow)
    return out


def quarter_turn(mv):
    """The records with every src replaced by dst - (-dy, dx) (consequence E); the caller sees to it that this stays
    inside int16."""
    dx, dy = dm.displacement(mv)
    out = mv.copy()
    sx, sy = mv["dst_x"].astype(np.int64) + dy, mv["dst_y"].astype(np.int64) - dx
    assert (np.abs(sx) < 32768).all() and (np.abs(sy) < 32768).all()
    out["src_x"], out["src_y"] = sx, sy
    return out


def turned(motion):
    """What consequence E says `motion` becomes under quarter_turn (heading: only where the maximum of n is unique)."""
    out = motion.copy()
    out["n"] = np.roll(motion["n"], 2, axis=-1)
    out["sum_dx"], out["sum_dy"] = -motion["sum_dy"], motion["sum_dx"]
    h = motion["heading"].astype(np.int64)
    out["heading"] = np.where(h == NONE, NONE, (h + 2) & 7)
    return out


def unique_max(motion):
    n = motion["n"].astype(np.int64)
    return (n == n.max(axis=-1, keepdims=True)).sum(axis=-1) == 1


def same(a, b):
    """Exact equality of two arrays of one dtype and shape, structured ones included (no field is padded)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
