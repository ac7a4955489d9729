"""Inputs of the persistence tests (tests/test_persist_host.py, tests/test_gpu_persist.py): the worked cases of
include/mtgpu_persist.h with their hand values, the random generator of both tiers, and the seam, shape and end-to-end
batches of the GPU tier.  Everything is generated from seeds; the expected values of the generated batches come from
tests/persist_model.py, never from the GPU.  A case is a dict: flags uint8 [F], soff uint64 [S + 1], sd uint8 [F] or
None, box BLOB_BOX [F] or None, and the settings min_run, max_dropout, reach."""
import numpy as np

from mvtrim_amd import _abi

NO_LIMIT = 0xFFFFFFFF
GRID_W, GRID_H = 120, 68
BOX = _abi.BLOB_BOX_DTYPE


def case(flags, soff=None, sd=None, box=None, min_run=1, max_dropout=0, reach=1):
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    soff = np.array([0, len(flags)] if soff is None else soff, dtype=np.uint64)
    return dict(flags=flags, soff=soff, sd=None if sd is None else np.ascontiguousarray(sd, dtype=np.uint8),
                box=None if box is None else boxes(box), min_run=int(min_run), max_dropout=int(max_dropout), reach=int(reach))


def boxes(rows):
    """BLOB_BOX [F] from rows of (x0, y0, x1, y1) or from a BLOB_BOX array."""
    rows = np.asarray(rows)
    if rows.dtype == BOX:
        return np.ascontiguousarray(rows)
    return np.ascontiguousarray(rows, dtype=np.uint16).reshape(-1, 4).copy().view(BOX).reshape(-1)


def classes(text):
    """'M M Q M T' -> (flags, has_sd): M = flagged, Q = quiet with side data, T = quiet key frame without."""
    t = text.split()
    return (np.array([1 if c == "M" else 0 for c in t], dtype=np.uint8), np.array([0 if c == "T" else 1 for c in t], dtype=np.uint8))


# ------------------------------------------------------------------ the worked cases, checked by hand

_F9, _SD9 = classes("M M Q M T M Q Q M")
_B3 = [(2, 2, 3, 3), (5, 2, 6, 3), (9, 2, 9, 3)]

# name -> (case, run, pos, flags_out)
WORKED = {
    "dropout1": (case(_F9, sd=_SD9, max_dropout=1, min_run=2), [4, 4, 0, 4, 0, 4, 0, 0, 1], [1, 2, 0, 3, 0, 4, 0, 0, 1], [1, 1, 0, 1, 0, 1, 0, 0, 0]),
    "dropout0": (case(_F9, sd=_SD9, max_dropout=0, min_run=2), [2, 2, 0, 2, 0, 2, 0, 0, 1], [1, 2, 0, 1, 0, 2, 0, 0, 1], [1, 1, 0, 1, 0, 1, 0, 0, 0]),
    "no_has_sd": (case(_F9, max_dropout=0, min_run=2), [2, 2, 0, 1, 0, 1, 0, 0, 1], [1, 2, 0, 1, 0, 1, 0, 0, 1], [1, 1, 0, 0, 0, 0, 0, 0, 0]),
    "reach1": (case([1, 1, 1], box=_B3, reach=1, min_run=2), [1, 1, 1], [1, 1, 1], [0, 0, 0]),
    "reach2": (case([1, 1, 1], box=_B3, reach=2, min_run=2), [2, 2, 1], [1, 2, 1], [1, 1, 0]),
    "reach3": (case([1, 1, 1], box=_B3, reach=3, min_run=2), [3, 3, 3], [1, 2, 3], [1, 1, 1]),
}


def embed(c, index=3, n_streams=5, seed=11):
    """The case's one stream as stream `index` of `n_streams`: the others are random streams of 0 .. 40 frames with the
    same kinds of inputs.  Returns (case, slice of the embedded stream)."""
    assert len(c["soff"]) == 2 and int(c["soff"][0]) == 0 and int(c["soff"][1]) == len(c["flags"])
    rng = np.random.RandomState(seed)
    parts = []
    for s in range(n_streams):
        if s == index:
            parts.append((c["flags"], c["sd"], c["box"]))
        else:
            n = int(rng.randint(0, 41))
            fl, sd, bx = random_stream(rng, n, float(rng.uniform(0.2, 0.9)), int(rng.randint(2, 9)), True)
            parts.append((fl, sd if c["sd"] is not None else None, bx if c["box"] is not None else None))
    lens = [len(p[0]) for p in parts]
    soff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    out = dict(c)
    out["flags"] = np.concatenate([p[0] for p in parts])
    out["sd"] = None if c["sd"] is None else np.concatenate([p[1] for p in parts])
    out["box"] = None if c["box"] is None else np.concatenate([p[2] for p in parts])
    out["soff"] = soff
    return out, slice(int(soff[index]), int(soff[index + 1]))


# ------------------------------------------------------------------ the random generator of both tiers

def random_stream(rng, n, density, key_every, with_box, strict_keys=True):
    """One stream: M with probability `density`; every key_every-th frame (0: never) is a key frame without side data,
    and unflagged when strict_keys; boxes on a GRID_W x GRID_H grid — mostly the last box moved by a few cells, sometimes
    a fresh one, sometimes the all-0xFFFF box."""
    fl = (rng.random_sample(n) < density).astype(np.uint8)
    sd = np.ones(n, dtype=np.uint8)
    if key_every:
        sd[::key_every] = 0
        if strict_keys:
            fl[::key_every] = 0
    bx = None
    if with_box:
        rows = np.full((n, 4), 0xFFFF, dtype=np.int64)
        x0, y0, w, h = 40, 30, 3, 2
        for f in range(n):
            u = rng.random_sample()
            if u < 0.15:
                x0, y0 = int(rng.randint(0, GRID_W)), int(rng.randint(0, GRID_H))
                w, h = int(rng.randint(0, 12)), int(rng.randint(0, 8))
            else:
                x0 = int(np.clip(x0 + rng.randint(-4, 5), 0, GRID_W - 1))
                y0 = int(np.clip(y0 + rng.randint(-3, 4), 0, GRID_H - 1))
            if fl[f] and u > 0.93:
                continue                                   # a flagged frame without a blob: links to nothing
            if fl[f] or u < 0.5:                           # (quiet frames carry boxes too: they must not matter)
                rows[f] = (x0, y0, min(x0 + w, GRID_W - 1), min(y0 + h, GRID_H - 1))
        bx = boxes(rows)
    return fl, sd, bx


def long_stream(n, seed=31):
    """One long stream, generated without a Python loop: M density 0.7, a key frame every 30, a box that wanders by at
    most two cells a frame and jumps now and then, one flagged frame in twenty without a blob."""
    rng = np.random.RandomState(seed)
    fl = (rng.random_sample(n) < 0.7).astype(np.uint8)
    sd = np.ones(n, dtype=np.uint8)
    sd[::30] = 0
    fl[::30] = 0
    jump = rng.random_sample(n) < 0.02
    x0 = (40 + np.cumsum(rng.randint(-2, 3, size=n) + jump * rng.randint(-60, 61, size=n))) % (GRID_W - 4)
    y0 = (30 + np.cumsum(rng.randint(-2, 3, size=n) + jump * rng.randint(-30, 31, size=n))) % (GRID_H - 3)
    rows = np.stack([x0, y0, x0 + 3, y0 + 2], axis=1)
    rows[rng.random_sample(n) < 0.05] = 0xFFFF
    return fl, sd, boxes(rows)


def random_case(seed, max_streams=4, max_len=300, with_box=None, with_sd=None):
    """Draw `seed`: 1 .. max_streams streams of 0 .. max_len frames, M density 0.05 .. 0.95, a key frame every 2 .. 30
    frames or never, with or without boxes and has_sd, and settings from the ranges where they bite."""
    rng = np.random.RandomState(1000 + seed)
    ns = int(rng.randint(1, max_streams + 1))
    with_box = bool(rng.randint(0, 2)) if with_box is None else with_box
    with_sd = bool(rng.randint(0, 2)) if with_sd is None else with_sd
    parts = []
    for _ in range(ns):
        n = int(rng.randint(0, max_len + 1))
        key = int(rng.randint(2, 31)) if rng.random_sample() < 0.8 else 0
        parts.append(random_stream(rng, n, float(rng.uniform(0.05, 0.95)), key, with_box, strict_keys=seed % 5 != 0))
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    flags = np.concatenate([p[0] for p in parts])
    flags = np.where(flags != 0, rng.choice([1, 1, 2, 255], size=len(flags)), 0).astype(np.uint8)
    return case(flags, soff, np.concatenate([p[1] for p in parts]) if with_sd else None,
                np.concatenate([p[2] for p in parts]) if with_box else None, min_run=int(rng.choice([0, 1, 2, 3, 5])),
                max_dropout=int(rng.choice([0, 0, 1, 2, 5, NO_LIMIT])), reach=int(rng.choice([0, 1, 2, 5, 20, 65535])))


def single_streams(c):
    """The case cut into one case per stream (consequence G)."""
    out = []
    for s in range(len(c["soff"]) - 1):
        sl = slice(int(c["soff"][s]), int(c["soff"][s + 1]))
        one = dict(c)
        one.update(flags=c["flags"][sl], soff=np.array([0, sl.stop - sl.start], dtype=np.uint64),
                   sd=None if c["sd"] is None else c["sd"][sl], box=None if c["box"] is None else c["box"][sl])
        out.append((sl, one))
    return out


# ------------------------------------------------------------------ seams (GPU tier): one stream of 3T + 5 frames

def seam_positions(T, workgroup, W=64):
    return [W - 1, W, W + 1, workgroup, T - 1, T, T + 1, 2 * T]


def seam_cases(T, workgroup, W=64):
    """name -> case.  Around each seam position k: a run that starts at k, a run that ends at k - 1, a Q-streak of exactly
    max_dropout frames and one of max_dropout + 1 across k, and a previous M frame a whole tile back whose box decides
    the link.  Then the streams that are one class throughout."""
    n = 3 * T + 5
    out = {}
    for k in seam_positions(T, workgroup, W):
        fl = np.zeros(n, dtype=np.uint8)
        fl[k - 10:k - 2] = 1
        fl[k:k + 7] = 1
        out[f"start@{k}"] = case(fl, max_dropout=1)            # Q at k - 2, k - 1: the run starts at k
        fl = np.zeros(n, dtype=np.uint8)
        fl[k - 9:k] = 1
        fl[k + 3:k + 5] = 1
        out[f"end@{k}"] = case(fl, max_dropout=2)              # three Q frames behind k - 1
        for md in (0, 1, 5):
            for d in (md, md + 1):
                a = k - d // 2                                  # the streak [a, a + d) lies across k (d >= 2) or touches it
                fl = np.zeros(n, dtype=np.uint8)
                fl[a - 6:a] = 1
                fl[a + d:a + d + 6] = 1
                out[f"streak{d}/{md}@{k}"] = case(fl, max_dropout=md)
        # M at k and at k + T, only T frames (all key frames) or only Q frames (no dropout limit) between
        for quiet, md in (("T", 0), ("Q", NO_LIMIT)):
            for link in (True, False):
                fl = np.zeros(n, dtype=np.uint8)
                fl[k] = fl[k + T] = 1
                sd = np.ones(n, dtype=np.uint8)
                if quiet == "T":
                    sd[k + 1:k + T] = 0
                rows = np.full((n, 4), 0xFFFF, dtype=np.int64)
                rows[k + 1:k + T] = (0, 0, 119, 67)             # boxes of quiet frames: never looked at
                rows[k] = (10, 10, 12, 12)
                rows[k + T] = (14, 10, 16, 12) if link else (15, 10, 16, 12)
                out[f"tile-back-{quiet}-{'linked' if link else 'apart'}@{k}"] = case(fl, sd=sd, box=rows, max_dropout=md, reach=2)
    ones, zeros = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    ends = zeros.copy()
    ends[0] = ends[-1] = 1
    sd = zeros.copy()
    sd[0] = sd[-1] = 1
    out["whole-stream-run"] = case(ends, sd=sd)                 # first and last frame, key frames between: one run of 2
    out["all-M"] = case(ones, sd=ones)
    out["all-Q"] = case(zeros, sd=ones)
    out["all-T"] = case(zeros, sd=zeros)
    return out


# ------------------------------------------------------------------ stream shapes (GPU tier)

def shape_lengths(T, W=64, seed=5):
    rng = np.random.RandomState(seed)
    return [0, 1, 2, W, T, T + 1, 0, 0] + [int(v) for v in rng.randint(1, 4, size=64)]


def shapes_case(T, W=64, head=3, tail=5, seed=5):
    """The stream lengths of shape_lengths back to back, `head` frames in front of stream_off[0] and `tail` frames
    behind stream_off[S]: those must read 0 in every output whatever they hold."""
    rng = np.random.RandomState(seed + 1)
    lens = shape_lengths(T, W, seed)
    soff = (head + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    n = int(soff[-1]) + tail
    fl, sd, bx = random_stream(rng, n, 0.6, 7, True)
    fl[:head] = 1
    fl[n - tail:] = 1
    return case(fl, soff, sd, bx, min_run=2, max_dropout=1, reach=3)


# ------------------------------------------------------------------ consequence E (GPU tier)

def sweep_case(seed=3, n_streams=3, length=400, fps=10.0):
    """Three streams with pts at 10 fps: (case, pts float64 [F])."""
    rng = np.random.RandomState(seed)
    parts = [random_stream(rng, length, d, 30, False) for d in (0.15, 0.5, 0.85)][:n_streams]
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    pts = np.concatenate([np.arange(len(p[0]), dtype=np.float64) / fps for p in parts])
    return case(np.concatenate([p[0] for p in parts]), soff, np.concatenate([p[1] for p in parts]), max_dropout=1), pts


# ------------------------------------------------------------------ end to end on synth (GPU tier)

E2E_FRAMES = 200
E2E_EVENT = (120, 150)
E2E_FLASHES = (45, 85, 119, 165)
E2E_KEPT = list(range(121, 150))       # the event's frames with side data: frame 120 is a key frame


def e2e_stream():
    """A 1080p stream (one record per cell, a key frame every 30) with one object moving through frames 120 .. 149 and
    single-frame flashes elsewhere in the picture — one of them in the frame before the event's key frame.  Returns
    (params, mv, frame_off, has_sd)."""
    import mvtrim_amd as m
    from mvtrim_amd import synth
    spec = synth.spec_1080p(seed=4, sub=1, salt_p=0.0)
    spec.events = [synth.Event(E2E_EVENT[0], E2E_EVENT[1], 40, 30, 4, 3, 8, 2)]
    spec.events += [synth.Event(f, f + 1, 100 - 10 * i, 12 + 9 * i, 3, 3, 9, 2) for i, f in enumerate(E2E_FLASHES)]
    mv, off, _pts, sd = synth.gen_stream(spec, E2E_FRAMES)
    return m.ScanParams.from_config(1920, 1080, vectors_needed=1, clusters_needed=1), mv, off, sd


# ------------------------------------------------------------------ the C example's stream

def example_flags(n=300):
    """examples/persist_example.c: a key frame every 30, a single-frame flash every 40 frames (off the key frames), one
    object for frames 120 .. 149 (its key frames stay unflagged)."""
    fl = np.zeros(n, dtype=np.uint8)
    sd = np.ones(n, dtype=np.uint8)
    sd[::30] = 0
    fl[15::40] = 1
    fl[120:150] = 1
    fl[sd == 0] = 0
    return fl, sd
