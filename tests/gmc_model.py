"""A numpy restatement of include/mtgpu_gmc.h, steps 1-5 (TEST ONLY): the counted records, the two histograms, the mode
walk 0, -1, +1, -2, +2, ..., the support test, the residual vote and the centres of src/motion_scanner.cpp:262-292.
Written with exact Python / int64 arithmetic; tests/test_gmc_host.py holds it against the hand values of
tests/gmc_inputs.py and, through consequence C, against the unchanged oracle."""
import numpy as np

from mvtrim_amd import _abi


def walk(max_shift):
    """The candidates in the order of step 3."""
    out = [0]
    for v in range(1, max_shift + 1):
        out += [-v, v]
    return out


def displacements(mv):
    return (mv["dst_x"].astype(np.int64) - mv["src_x"].astype(np.int64), mv["dst_y"].astype(np.int64) - mv["src_y"].astype(np.int64))


def cells(p, mv):
    return mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift


def counted(p, mv):
    """Step 1: the bounds test of :262."""
    cx, cy = cells(p, mv)
    m = p.vertical_margin
    return (cx >= 0) & (cx < p.grid_w) & (cy >= m) & (cy < p.grid_h - m)


def mode_of(d, max_shift):
    """Steps 2 and 3 for one axis: (mode, its count) over the displacements d of the counted records."""
    best_v, best_n = 0, 0
    for v in walk(max_shift):
        n = int((d == v).sum())
        if n > best_n:
            best_v, best_n = v, n
    return best_v, best_n


def estimate(p, mv, max_shift, min_share_q8):
    """Steps 1-4 of one frame WITH side data -> dict of the mt_gmc_info fields."""
    inside = counted(p, mv)
    n_in = int(inside.sum())
    dx, dy = displacements(mv)
    mx, nx = mode_of(dx[inside], max_shift)
    my, ny = mode_of(dy[inside], max_shift)
    gx = mx if nx * 256 >= min_share_q8 * n_in else 0
    gy = my if ny * 256 >= min_share_q8 * n_in else 0
    return dict(gx=gx, gy=gy, mode_x=mx, mode_y=my, n_in=n_in, n_x=nx, n_y=ny)


def threshold_int(thr):
    """The smallest integer magnitude that is NOT below the double threshold (:251 `mag < thr`; NaN keeps everything)."""
    thr = float(thr)
    if thr != thr or thr <= 0.0:
        return 0
    if thr == float("inf"):
        return None
    return int(np.ceil(thr))


def residual_centres(p, mv, gx, gy):
    """Step 5: the centre count of one frame WITH side data, residuals of (gx, gy), exact integers."""
    gw, gh, m = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(m, gh):max(gh - m, min(m, gh))] = True
    votes = np.zeros((gh, gw), dtype=np.int64)
    t = threshold_int(p.mv_threshold_sq)
    if len(mv) and t is not None:
        dx, dy = displacements(mv)
        rx, ry = dx - gx, dy - gy
        mag = rx * rx + ry * ry                                   # < 2^34: exact in int64
        cx, cy = cells(p, mv)
        ok = counted(p, mv) & (mag >= t)
        np.add.at(votes, (cy[ok], cx[ok]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    return int((act & nb & rows)[:, 1:gw - 1].sum())


def gmc_frame(p, mv, max_shift, min_share_q8):
    """(centres, info dict) of one frame WITH side data."""
    info = estimate(p, mv, max_shift, min_share_q8)
    return residual_centres(p, mv, info["gx"], info["gy"]), info


def has_side_data(off, sd):
    return np.asarray(sd).astype(bool) if sd is not None else np.diff(np.asarray(off).astype(np.int64)) > 0


def gmc_batch(p, mv, off, sd, max_shift, min_share_q8):
    """(flags uint8 [F], centres uint32 [F], info GMC_INFO_DTYPE [F]) of a batch; 0 everywhere without side data."""
    F = len(off) - 1
    has = has_side_data(off, sd)
    centres = np.zeros(F, dtype=np.uint32)
    info = np.zeros(F, dtype=_abi.GMC_INFO_DTYPE)
    for f in range(F):
        if has[f]:
            c, i = gmc_frame(p, mv[int(off[f]):int(off[f + 1])], max_shift, min_share_q8)
            centres[f] = c
            for k, v in i.items():
                info[k][f] = v
    return (centres >= max(1, p.clusters_needed)).astype(np.uint8), centres, info


def shift_src(mv, off, ax, ay):
    """A copy of the batch with (ax[f], ay[f]) added to the src of every record of frame f.  None where an int16
    would overflow."""
    fr = np.repeat(np.arange(len(off) - 1), np.diff(np.asarray(off).astype(np.int64)))
    lo = int(off[0])
    sx = mv["src_x"][lo:int(off[-1])].astype(np.int64) + np.asarray(ax, dtype=np.int64)[fr]
    sy = mv["src_y"][lo:int(off[-1])].astype(np.int64) + np.asarray(ay, dtype=np.int64)[fr]
    if len(sx) and (min(sx.min(), sy.min()) < -32768 or max(sx.max(), sy.max()) > 32767):
        return None
    out = mv.copy()
    out["src_x"][lo:int(off[-1])] = sx
    out["src_y"][lo:int(off[-1])] = sy
    return out
