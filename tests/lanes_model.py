"""Direction planes (include/mtgpu_lanes.h) restated in numpy on top of tests/dir_model.py: the plane scan, the record
filter of its consequence C that lets the unchanged oracle supply expected centre counts, and the flow map.
tests/test_lanes_host.py holds them against each other without a GPU; tests/test_gpu_lanes.py compares the kernels with
the model, exactly."""
import numpy as np

from mvtrim_amd import direction

import dir_model as dm
import oracle_binding as ob


def cells(p, mv):
    """(gx, gy) int64 per record: the destination cell (dst >> shift; may lie outside the grid)."""
    return mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift


def analysed(p, mv):
    """bool per record: the bounds test of src/motion_scanner.cpp:262 alone."""
    gx, gy = cells(p, mv)
    return (gx >= 0) & (gx < p.grid_w) & (gy >= p.vertical_margin) & (gy < p.grid_h - p.vertical_margin)


def allowed(p, mv, plane):
    """bool per record: a record without a sector passes; a record inside the analysed rows passes iff bit `sector` of
    its destination cell's byte is set.  Records outside the analysed rows read no byte (they never count) and pass."""
    plane = np.asarray(plane)
    assert plane.shape == (p.grid_h, p.grid_w) and plane.dtype == np.uint8
    sec = direction.sector_of(*dm.displacement(mv))
    gx, gy = cells(p, mv)
    ins = analysed(p, mv)
    byte = np.full(len(mv), 0xFF, dtype=np.int64)
    byte[ins] = plane[gy[ins], gx[ins]]
    return (sec < 0) | (((byte >> np.maximum(sec, 0)) & 1) != 0)


def frame_np(p, mv, plane):
    """(centres, rose int64 [8]) of one frame WITH side data, as dir_model.frame_np with the plane's test."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    ok = dm.counting(p, mv)
    sec = direction.sector_of(*dm.displacement(mv))
    rose = np.bincount(sec[ok & (sec >= 0)], minlength=8).astype(np.int64)
    vote = ok & allowed(p, mv, plane)
    gx, gy = cells(p, mv)
    votes = np.zeros((gh, gw), dtype=np.int64)
    np.add.at(votes, (gy[vote], gx[vote]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    return int((act & nb & rows)[:, 1:gw - 1].sum()), rose


def frame_planes(n_frames, planes, soff=None):
    """int per frame: the index of its plane in `planes` ([S, gh, gw], or [gh, gw] without soff), -1 for a frame that
    belongs to no stream."""
    planes = np.asarray(planes)
    if soff is None:
        assert planes.ndim == 2
        return np.zeros(n_frames, dtype=np.int64)
    assert planes.ndim == 3 and len(planes) == len(soff) - 1
    st = dm.stream_of_frames(soff, n_frames)
    return np.where((st >= 0) & (st < len(planes)), st, -1)


def _plane(planes, i):
    planes = np.asarray(planes)
    return planes if planes.ndim == 2 else planes[i]


def model_batch(p, mv, off, sd, planes, soff=None):
    """(flags uint8 [F], centres uint32 [F], rose uint32 [F, 8]) of a batch."""
    F = len(off) - 1
    has, fp = dm.has_side_data(off, sd), frame_planes(F, planes, soff)
    c, rose = np.zeros(F, dtype=np.uint32), np.zeros((F, 8), dtype=np.uint32)
    for f in range(F):
        if has[f] and fp[f] >= 0:
            c[f], rose[f] = frame_np(p, mv[int(off[f]):int(off[f + 1])], _plane(planes, fp[f]))
    return (c >= max(1, p.clusters_needed)).astype(np.uint8), c, rose


def filter_records(p, mv, off, planes, soff=None):
    """(mv, off) with every record removed whose sector its destination cell forbids (consequence C).  A frame that
    belongs to no stream loses every record."""
    F = len(off) - 1
    fp = frame_planes(F, planes, soff)
    parts, counts = [], []
    for f in range(F):
        part = mv[int(off[f]):int(off[f + 1])]
        part = part[:0] if fp[f] < 0 else part[allowed(p, part, _plane(planes, fp[f]))]
        parts.append(part)
        counts.append(len(part))
    new_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return np.ascontiguousarray(np.concatenate(parts) if parts else mv[:0]), new_off


def oracle_batch(p, mv, off, sd, planes, soff=None):
    """(flags, centres) through consequence C: the unchanged oracle on the filtered records, has_sd passed explicitly and
    unchanged.  Frames that belong to no stream: 0."""
    F = len(off) - 1
    has = dm.has_side_data(off, sd).astype(np.uint8)
    fmv, foff = filter_records(p, mv, off, planes, soff)
    fl, ce = ob.scan_centres(p, fmv, foff, has, nthreads=4)
    fl, ce = fl.copy(), ce.copy()
    orphan = frame_planes(F, planes, soff) < 0
    fl[orphan], ce[orphan] = 0, 0
    return fl, ce


def flow_map(p, mv, off, sd, soff):
    """uint32 [S, 8, gh, gw]: the counting records with a sector per stream, sector and destination cell, over the frames
    with side data.  A frame outside every stream counts nowhere."""
    F, S = len(off) - 1, len(soff) - 1
    has = dm.has_side_data(off, sd)
    st = dm.stream_of_frames(soff, F)
    flow = np.zeros((S, 8, p.grid_h, p.grid_w), dtype=np.uint32)
    for f in range(F):
        if not has[f] or st[f] < 0 or st[f] >= S:
            continue
        part = mv[int(off[f]):int(off[f + 1])]
        sec = direction.sector_of(*dm.displacement(part))
        take = dm.counting(p, part) & (sec >= 0)
        gx, gy = cells(p, part)
        np.add.at(flow[st[f]], (sec[take], gy[take], gx[take]), 1)
    return flow


def zones_keep(plane):
    """bool [gh, gw] of consequence E: keep = (byte == 0xFF), for a plane whose bytes are all 0x00 or 0xFF."""
    plane = np.asarray(plane)
    assert np.isin(plane, (0x00, 0xFF)).all()
    return plane == 0xFF
