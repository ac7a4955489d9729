"""Object tracks (include/mtgpu_tracks.h) as a plain sequential loop per stream over the header's definitions: frame
classes M / T / Q, p(f), q(f), present entries, pred, age, id, len, track, flags_out.  No scan, no cleverness: one pass
over the frames gives pred, age and id; the largest age per id gives len.  Checker only."""
import numpy as np

from persist_model import linked

NO_PRED = 0xFF
NO_ID = 0xFFFFFFFF
K_MAX = 16


def tracks(flags, lists, stream_off, has_sd=None, min_cells=1, max_dropout=0, reach=1, min_track=1):
    """flags: [F] (non-zero: M); lists: OBJECT_DTYPE [F, k]; stream_off: [S + 1]; has_sd: [F] or None.  Returns {"pred":
    uint8 [F, k], "age" / "id" / "len": uint32 [F, k], "track": uint32 [F], "flags": uint8 [F]}; entries that are not
    present and frames outside the streams read the empty values."""
    flags = np.asarray(flags)
    lists = np.asarray(lists)
    n, k = lists.shape
    assert len(flags) == n and 1 <= k <= K_MAX
    soff = [min(int(v), n) for v in np.asarray(stream_off).tolist()]
    cells = lists["cells"].astype(np.int64).tolist()
    box = np.stack([lists[c] for c in ("x0", "y0", "x1", "y1")], axis=2).astype(np.int64).tolist()
    need_cells, need_track = max(1, int(min_cells)), max(1, int(min_track))
    pred = np.full((n, k), NO_PRED, dtype=np.uint8)
    age = np.zeros((n, k), dtype=np.uint32)
    ident = np.full((n, k), NO_ID, dtype=np.uint32)
    length = np.zeros((n, k), dtype=np.uint32)
    track = np.zeros(n, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint8)
    depth = {}                 # id -> the largest age that carries it
    inside = []
    for s in range(len(soff) - 1):
        prev = None            # p(f): the previous M frame of the stream
        quiet = 0              # Q frames since prev
        for f in range(soff[s], max(soff[s], soff[s + 1])):
            inside.append(f)
            if flags[f] != 0:
                for j in range(k):
                    if cells[f][j] < need_cells:
                        continue                                   # not present
                    pr = None
                    if prev is not None and quiet <= max_dropout:
                        for i in range(k):
                            if cells[prev][i] >= need_cells and linked(box[prev][i], box[f][j], reach):
                                pr = i
                                break
                    if pr is None:
                        age[f, j], ident[f, j] = 1, f * k + j
                    else:
                        pred[f, j], age[f, j], ident[f, j] = pr, age[prev, pr] + 1, ident[prev, pr]
                    depth[int(ident[f, j])] = max(depth.get(int(ident[f, j]), 0), int(age[f, j]))
                prev, quiet = f, 0
            elif has_sd is not None and has_sd[f] == 0:
                pass           # T: transparent
            else:
                quiet += 1     # Q
    for f in inside:
        for j in range(k):
            if ident[f, j] != NO_ID:
                length[f, j] = depth[int(ident[f, j])]
        track[f] = length[f].max()
        out[f] = 1 if flags[f] != 0 and track[f] >= need_track else 0
    return {"pred": pred, "age": age, "id": ident, "len": length, "track": track, "flags": out}
