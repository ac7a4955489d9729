"""The numpy model of the per-stream activity maps (include/mtgpu_activity.h): histogram, saturate at 255, `>= vn`,
shifted planes — the style of np_model.check_frame_np, which it extends by vn == 0 with a margin, analysed-rows-only for
the active plane and contribution by min_centres.  Shared by tests/test_gpu_activity.py, the derived kernels' limit
shapes and their soak; it needs no GPU.  assert_oracle_identities ties the model (or a device's maps) to the oracle."""
import numpy as np

import oracle_binding as ob


def frame_planes(p, mv):
    """(active bool [gh, gw], centre bool [gh, gw]) of one frame WITH side data (src/motion_scanner.cpp:242-292)."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    votes = np.zeros((gh, gw), dtype=np.int64)
    if len(mv):
        dx = mv["dst_x"].astype(np.int64) - mv["src_x"].astype(np.int64)
        dy = mv["dst_y"].astype(np.int64) - mv["src_y"].astype(np.int64)
        keep = ~((dx * dx + dy * dy).astype(np.float64) < p.mv_threshold_sq)
        gx = mv["dst_x"].astype(np.int64) >> p.block_shift
        gy = mv["dst_y"].astype(np.int64) >> p.block_shift
        keep &= (gx >= 0) & (gx < gw) & (gy >= mg) & (gy < gh - mg)
        np.add.at(votes, (gy[keep], gx[keep]), 1)
    votes = np.minimum(votes, 255)                                  # u8 saturation
    act = votes >= (p.vectors_needed & 0xFF)                        # vn == 0: every cell of the grid, masked rows too
    nb = np.zeros_like(act)
    nb[:, 1:] |= act[:, :-1]
    nb[:, :-1] |= act[:, 1:]
    nb[1:, :] |= act[:-1, :]
    nb[:-1, :] |= act[1:, :]
    rows = np.zeros(gh, dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    centre = act & nb & rows[:, None]
    centre[:, 0] = False
    centre[:, gw - 1:] = False
    return act & rows[:, None], centre                              # the active plane: analysed rows only


def model_maps(p, mv, off, sd, stream_off, min_centres):
    """(active uint32 [S, gh, gw], centre uint32 [S, gh, gw], frames uint32 [S], per-frame centre counts int64 [F])."""
    S, F = len(stream_off) - 1, len(off) - 1
    active = np.zeros((S, p.grid_h, p.grid_w), dtype=np.uint32)
    centre = np.zeros_like(active)
    frames = np.zeros(S, dtype=np.uint32)
    counts = np.zeros(F, dtype=np.int64)
    for s in range(S):
        for f in range(int(stream_off[s]), int(stream_off[s + 1])):
            a, b = int(off[f]), int(off[f + 1])
            if not (sd[f] if sd is not None else b > a):
                continue
            act, cen = frame_planes(p, mv[a:b])
            counts[f] = int(cen.sum())
            if counts[f] >= min_centres:
                active[s] += act
                centre[s] += cen
                frames[s] += 1
    return active, centre, frames, counts


def assert_oracle_identities(p, mv, off, sd, stream_off, min_centres, centre, frames, what):
    """The model's (or the device's) centre plane and frame counts against the oracle's per-frame centre counts."""
    oc = ob.scan_centres(p, mv, off, sd, nthreads=4)[1].astype(np.int64)
    has = np.asarray(sd).astype(bool) if sd is not None else np.diff(np.asarray(off).astype(np.int64)) > 0
    take = has & (oc >= min_centres)
    for s in range(len(stream_off) - 1):
        a, b = int(stream_off[s]), int(stream_off[s + 1])
        assert int(centre[s].sum(dtype=np.uint64)) == int(oc[a:b][take[a:b]].sum()), (what, "centre sum of stream", s)
        assert int(frames[s]) == int(take[a:b].sum()), (what, "frames of stream", s)
    return oc
