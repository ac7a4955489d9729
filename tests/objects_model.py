"""numpy restatement of the object scan (include/mtgpu_objects.h): blobs_model.centre_plane and blobs_model.label — the
active plane, the centres and the flood fill of the blob scan's model, unchanged — then a sort of the components by
(-cells, first).  tests/test_objects_host.py holds it to hand-derived planes and, entry 0, to blobs_model.blob_stats."""
import numpy as np

import mvtrim_amd as m

import blobs_model as bm
import zones_inputs as zi

OBJECT_DTYPE = m._abi.OBJECT_DTYPE
K_MAX = m._abi.OBJECTS_MAX
EMPTY = (0, 0xFFFFFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)


def ranked(cen):
    """Every blob of a centre plane (bool [gh, gw]) as (cells, first, x0, y0, x1, y1), in list order: cells descending,
    then first — the smallest y * gw + x of its cells — ascending."""
    lab = bm.label(cen)
    n = int(lab.max())
    gw = cen.shape[1]
    out = []
    for i in range(1, n + 1):
        ys, xs = np.nonzero(lab == i)
        out.append((len(xs), int((ys * gw + xs).min()), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())))
    return sorted(out, key=lambda b: (-b[0], b[1]))


def ranked_fast(cen, k):
    """(the first k entries of ranked(cen), every blob's cell count): the boxes are computed for the listed blobs only."""
    lab = bm.label(cen)
    n = int(lab.max())
    if n == 0:
        return [], np.zeros(0, dtype=np.int64)
    flat = lab.reshape(-1)
    sizes = np.bincount(flat, minlength=n + 1)[1:]
    idx = np.flatnonzero(flat)
    labs, where = np.unique(flat[idx], return_index=True)        # the first cell of label i in row-major order
    first = idx[where]
    assert labs.tolist() == list(range(1, n + 1))
    order = sorted(range(n), key=lambda i: (-int(sizes[i]), int(first[i])))[:k]
    out = []
    for i in order:
        ys, xs = np.nonzero(lab == i + 1)
        out.append((int(sizes[i]), int(first[i]), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())))
    return out, sizes


def entries(blobs, k):
    """The first k of `blobs` as OBJECT_DTYPE [k], empty entries behind them."""
    e = np.array([EMPTY] * k, dtype=OBJECT_DTYPE)
    for j, b in enumerate(blobs[:k]):
        e[j] = b
    return e


def model_batch(p, mv, off, sd, k=K_MAX, min_blob_cells=1, soff=None, keeps=None):
    """{"centres", "blobs", "objects": uint32 [F], "list": OBJECT_DTYPE [F, k]} of a batch; keeps: bool [S, gh, gw] with
    soff, or both None.  A frame without side data, and under a mask a frame behind the last stream, reads zeros and an
    empty list."""
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else np.zeros(F, dtype=np.int64)
    out = {n: np.zeros(F, dtype=np.uint32) for n in ("centres", "blobs", "objects")}
    out["list"] = np.array([[EMPTY] * k] * F, dtype=OBJECT_DTYPE).reshape(F, k)
    need = max(1, min_blob_cells)
    for f in range(F):
        if not has[f] or (keeps is not None and not 0 <= st[f] < len(keeps)):
            continue
        cen = bm.centre_plane(p, mv[int(off[f]):int(off[f + 1])], None if keeps is None else keeps[st[f]])
        top, sizes = ranked_fast(cen, k)
        out["centres"][f], out["blobs"][f], out["objects"][f] = int(cen.sum()), len(sizes), int((sizes >= need).sum())
        out["list"][f] = entries(top, k)
    return out


def objects_at(want, min_blob_cells):
    """objects[f] at another min_blob_cells from a model answer — where the list holds every blob (blobs <= k)."""
    assert (want["blobs"] <= want["list"].shape[1]).all()
    return (want["list"]["cells"] >= max(1, min_blob_cells)).sum(axis=1).astype(np.uint32)


def flags_np(p, centres, objects, min_objects):
    return ((np.asarray(centres) >= max(1, p.clusters_needed)) & (np.asarray(objects) >= max(1, min_objects))).astype(np.uint8)
