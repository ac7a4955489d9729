"""The direction filter (include/mtgpu_dir.h) restated in numpy, and the record filter of its consequence C that lets the
unchanged oracle supply expected centre counts.  tests/test_dir_host.py holds the two against each other without a GPU;
tests/test_gpu_dir.py compares the kernel with the model, exactly."""
import numpy as np

from mvtrim_amd import direction

import oracle_binding as ob


def displacement(mv):
    return (mv["dst_x"].astype(np.int64) - mv["src_x"], mv["dst_y"].astype(np.int64) - mv["src_y"])


def counting(p, mv):
    """bool per record: it passes the bounds test of src/motion_scanner.cpp:262 and the threshold of :251."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    dx, dy = displacement(mv)
    d2 = dx * dx + dy * dy
    gx, gy = mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift
    return ~(d2.astype(np.float64) < p.mv_threshold_sq) & (gx >= 0) & (gx < gw) & (gy >= mg) & (gy < gh - mg)


def passes(mv, allow):
    """bool per record: the direction test.  A record without a sector always passes."""
    sec = direction.sector_of(*displacement(mv))
    return (sec < 0) | (((int(allow) >> np.maximum(sec, 0)) & 1) != 0)


def frame_np(p, mv, allow):
    """(centres, rose int64 [8]) of one frame WITH side data: the votes of the counting records that pass the direction
    test; active = votes >= vn on the analysed rows and on their halo rows; a centre is an active cell of an analysed
    row, x in [1, gw - 2], with an active 4-neighbour; the rose counts every counting record with a sector."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    ok = counting(p, mv)
    sec = direction.sector_of(*displacement(mv))
    rose = np.bincount(sec[ok & (sec >= 0)], minlength=8).astype(np.int64)
    vote = ok & passes(mv, allow)
    gx, gy = mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift
    votes = np.zeros((gh, gw), dtype=np.int64)
    np.add.at(votes, (gy[vote], gx[vote]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    return int((act & nb & rows)[:, 1:gw - 1].sum()), rose


def has_side_data(off, sd):
    return np.asarray(sd).astype(bool) if sd is not None else np.diff(np.asarray(off).astype(np.int64)) > 0


def stream_of_frames(soff, n_frames):
    """Stream index per frame; len(soff) - 1 for a frame at or past soff[-1]."""
    return np.searchsorted(np.asarray(soff).astype(np.int64), np.arange(n_frames), side="right") - 1


def frame_allows(n_frames, allow, soff=None, allows=None):
    """int per frame: its allow byte, -1 for a frame that belongs to no stream."""
    if allows is None:
        return np.full(n_frames, int(allow), dtype=np.int64)
    st = stream_of_frames(soff, n_frames)
    a = np.asarray(allows).astype(np.int64)
    if len(a) == 0:
        return np.full(n_frames, -1, dtype=np.int64)
    return np.where((st >= 0) & (st < len(a)), a[np.clip(st, 0, len(a) - 1)], -1)


def model_batch(p, mv, off, sd, allow=0xFF, soff=None, allows=None):
    """(flags uint8 [F], centres uint32 [F], rose uint32 [F, 8]) of a batch."""
    F = len(off) - 1
    has, fa = has_side_data(off, sd), frame_allows(F, allow, soff, allows)
    c, rose = np.zeros(F, dtype=np.uint32), np.zeros((F, 8), dtype=np.uint32)
    for f in range(F):
        if has[f] and fa[f] >= 0:
            c[f], rose[f] = frame_np(p, mv[int(off[f]):int(off[f + 1])], int(fa[f]))
    return (c >= max(1, p.clusters_needed)).astype(np.uint8), c, rose


def filter_records(mv, off, allow=0xFF, soff=None, allows=None):
    """(mv, off) with every record removed whose sector its frame does not allow (consequence C).  A frame that belongs to
    no stream loses every record."""
    F = len(off) - 1
    fr = np.repeat(np.arange(F), np.diff(np.asarray(off).astype(np.int64)))
    mv = mv[int(off[0]):int(off[-1])]
    fa = frame_allows(F, allow, soff, allows)[fr]
    sec = direction.sector_of(*displacement(mv))
    take = (fa >= 0) & ((sec < 0) | (((np.maximum(fa, 0) >> np.maximum(sec, 0)) & 1) != 0))
    new_off = np.concatenate([[0], np.cumsum(np.bincount(fr[take], minlength=F))]).astype(np.uint64)
    return np.ascontiguousarray(mv[take]), new_off


def oracle_batch(p, mv, off, sd, allow=0xFF, soff=None, allows=None):
    """(flags, centres) through consequence C: the unchanged oracle on the filtered records, has_sd passed explicitly and
    unchanged.  Frames that belong to no stream: 0."""
    F = len(off) - 1
    has = has_side_data(off, sd).astype(np.uint8)
    fmv, foff = filter_records(mv, off, allow, soff, allows)
    fl, ce = ob.scan_centres(p, fmv, foff, has, nthreads=4)
    fl, ce = fl.copy(), ce.copy()
    orphan = frame_allows(F, allow, soff, allows) < 0
    fl[orphan], ce[orphan] = 0, 0
    return fl, ce


def counting_moving(p, mv, off, sd):
    """int64 [F]: the counting records with non-zero displacement of every frame with side data (consequence B)."""
    F = len(off) - 1
    has = has_side_data(off, sd)
    out = np.zeros(F, dtype=np.int64)
    for f in range(F):
        if has[f]:
            part = mv[int(off[f]):int(off[f + 1])]
            dx, dy = displacement(part)
            out[f] = int((counting(p, part) & ((dx != 0) | (dy != 0))).sum())
    return out
