"""numpy restatement of the blob scan (include/mtgpu_blobs.h): the active plane built as zones_inputs.zone_counts_np
builds it, the centre plane of src/motion_scanner.cpp:277-292, and the 4-connected components of the centres by plain
flood fill.  No scipy; tests/test_blobs_host.py holds the labelling against scipy.ndimage.label where scipy imports,
and the centre counts against the unchanged oracle."""
import numpy as np

import zones_inputs as zi

NO_BOX = (0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)


def active_plane(p, mv, keep=None):
    """bool [gh, gw] of one frame WITH side data: votes >= vn AND (keep OR the row is not analysed), and the analysed
    rows bool [gh, 1].  Line for line the plane of zones_inputs.zone_counts_np."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    d2 = (mv["dst_x"].astype(np.int64) - mv["src_x"]) ** 2 + (mv["dst_y"].astype(np.int64) - mv["src_y"]) ** 2
    gx, gy = mv["dst_x"].astype(np.int64) >> p.block_shift, mv["dst_y"].astype(np.int64) >> p.block_shift
    ok = ~(d2.astype(np.float64) < p.mv_threshold_sq) & (gx >= 0) & (gx < gw) & (gy >= 0) & (gy < gh)
    ok &= rows[np.clip(gy, 0, gh - 1), 0]
    votes = np.zeros((gh, gw), dtype=np.int64)
    np.add.at(votes, (gy[ok], gx[ok]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    if keep is not None:
        act = act & (np.asarray(keep, dtype=bool) | ~rows)
    return act, rows


def centre_plane(p, mv, keep=None):
    """bool [gh, gw]: active, on an analysed row, x in [1, gw - 2], with an active 4-neighbour."""
    act, rows = active_plane(p, mv, keep)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    cen = act & nb & rows
    cen[:, :1] = False
    cen[:, max(p.grid_w - 1, 0):] = False
    return cen


def label(cen):
    """int32 [gh, gw]: 0 = no centre, else 1 + the number of components whose first cell (row-major) comes earlier.
    Plain flood fill with a stack over the 4-neighbourhood."""
    gh, gw = cen.shape
    lab = np.zeros((gh, gw), dtype=np.int32)
    n = 0
    for y, x in zip(*np.nonzero(cen)):
        if lab[y, x]:
            continue
        n += 1
        lab[y, x] = n
        stack = [(int(y), int(x))]
        while stack:
            cy, cx = stack.pop()
            for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                if 0 <= ny < gh and 0 <= nx < gw and cen[ny, nx] and not lab[ny, nx]:
                    lab[ny, nx] = n
                    stack.append((ny, nx))
    return lab


def blob_stats(cen):
    """(centres, blobs, largest, (x0, y0, x1, y1)) of a centre plane.  Components are numbered by their first cell in
    row-major order, so argmax — the first maximum — is the tie rule: the blob holding the smallest y * gw + x."""
    lab = label(cen)
    n = int(lab.max())
    if n == 0:
        return 0, 0, 0, NO_BOX
    sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
    win = int(np.argmax(sizes)) + 1
    ys, xs = np.nonzero(lab == win)
    return int(cen.sum()), n, int(sizes[win - 1]), (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def frame_stats(p, mv, keep=None):
    return blob_stats(centre_plane(p, mv, keep))


def model_batch(p, mv, off, sd, soff=None, keeps=None):
    """{"centres", "blobs", "largest": uint32 [F], "box": uint16 [F, 4]} of a batch; keeps: bool [S, gh, gw] with soff, or
    both None.  A frame without side data, and under a mask a frame behind the last stream, reads 0 and an all-0xFFFF box."""
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else np.zeros(F, dtype=np.int64)
    out = {k: np.zeros(F, dtype=np.uint32) for k in ("centres", "blobs", "largest")}
    out["box"] = np.full((F, 4), 0xFFFF, dtype=np.uint16)
    for f in range(F):
        if not has[f] or (keeps is not None and not 0 <= st[f] < len(keeps)):
            continue
        c, b, g, box = frame_stats(p, mv[int(off[f]):int(off[f + 1])], None if keeps is None else keeps[st[f]])
        out["centres"][f], out["blobs"][f], out["largest"][f], out["box"][f] = c, b, g, box
    return out


def flags_np(p, centres, largest, min_blob_cells):
    return ((np.asarray(centres) >= max(1, p.clusters_needed)) & (np.asarray(largest) >= max(1, min_blob_cells))).astype(np.uint8)
