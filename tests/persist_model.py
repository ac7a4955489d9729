"""Temporal persistence (include/mtgpu_persist.h) as a plain sequential loop per stream over the header's definitions:
frame classes M / T / Q, p(f), q(f), brk(f), linked(A, B), runs, run / pos / flags_out.  No cleverness: one pass gives
brk and pos, a second pass over the runs gives run.  Checker only."""
import numpy as np

NO_BOX = (0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)


def linked(a, b, reach):
    """a, b: (x0, y0, x1, y1) as Python ints."""
    a, b = tuple(a), tuple(b)
    if a == NO_BOX or b == NO_BOX:
        return False
    ax0, ay0, ax1, ay1 = a
    bx0, by0, bx1, by1 = b
    return bx0 <= ax1 + reach and ax0 <= bx1 + reach and by0 <= ay1 + reach and ay0 <= by1 + reach


def persist(flags, stream_off, has_sd=None, box=None, min_run=1, max_dropout=0, reach=1):
    """flags: [F] (non-zero: M); stream_off: [S + 1]; has_sd: [F] or None; box: [F] rows of (x0, y0, x1, y1) (a
    structured BLOB_BOX array or an [F, 4] array) or None.  Returns {"flags": uint8 [F], "run": uint32 [F], "pos": uint32
    [F]}; frames outside the streams read 0."""
    flags = np.asarray(flags)
    n = len(flags)
    soff = [int(v) for v in np.asarray(stream_off).tolist()]
    if box is not None:
        box = np.asarray(box)
        if box.dtype.names:
            box = np.stack([box[k] for k in ("x0", "y0", "x1", "y1")], axis=1)
        box = box.astype(np.int64).tolist()
    run = np.zeros(n, dtype=np.uint32)
    pos = np.zeros(n, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint8)
    need = max(1, int(min_run))
    for s in range(len(soff) - 1):
        prev = None            # p(f): the previous M frame of the stream
        quiet = 0              # Q frames since prev
        members = []           # the M frames of the run that is open
        runs = []
        for f in range(soff[s], soff[s + 1]):
            if flags[f] != 0:
                brk = prev is None or quiet > max_dropout or (box is not None and not linked(box[prev], box[f], reach))
                if brk:
                    members = []
                    runs.append(members)
                members.append(f)
                pos[f] = len(members)
                prev, quiet = f, 0
            elif has_sd is not None and has_sd[f] == 0:
                pass           # T: transparent
            else:
                quiet += 1     # Q
        for members in runs:
            for f in members:
                run[f] = len(members)
                out[f] = 1 if len(members) >= need else 0
    return {"flags": out, "run": run, "pos": pos}
