"""Inputs of the tracks tests (tests/test_tracks_host.py, tests/test_gpu_tracks.py): hand-built object lists with every
expected value written out, the random generator of both tiers, and the seam, stream and end-to-end batches of the GPU
tier.  Everything is generated from seeds; the expected values of the generated batches come from tests/tracks_model.py,
never from the GPU.  A built case is a dict: flags uint8 [F], lists OBJECT_DTYPE [F, k], soff uint64 [S + 1], sd uint8
[F] or None, and the settings min_cells, max_dropout, reach, min_track."""
import numpy as np

from mvtrim_amd import _abi

import persist_inputs as pi

OBJ = _abi.OBJECT_DTYPE
NO_PRED, NO_ID = 0xFF, 0xFFFFFFFF
EMPTY = (0, 0xFFFFFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)
HAND_K = (1, 2, 15, 16)
NO_LIMIT = 0xFFFFFFFF


def obj(cells, x0, y0, x1, y1, first=None):
    """One list entry; `first` defaults to y0 * 120 + x0 (it plays no part in tracking)."""
    return (cells, y0 * 120 + x0 if first is None else first, x0, y0, x1, y1)


def lists_of(frames, k):
    """OBJECT_DTYPE [F, k] from per-frame lists of entries: cut to k, padded with EMPTY."""
    out = np.empty((len(frames), k), dtype=OBJ)
    for f, entries in enumerate(frames):
        row = (list(entries) + [EMPTY] * k)[:k]
        for j, e in enumerate(row):
            out[f, j] = e
    return out


def case(flags, lists, soff=None, sd=None, min_cells=1, max_dropout=0, reach=1, min_track=1):
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    soff = np.array([0, len(flags)] if soff is None else soff, dtype=np.uint64)
    return dict(flags=flags, lists=np.ascontiguousarray(lists, dtype=OBJ), soff=soff,
                sd=None if sd is None else np.ascontiguousarray(sd, dtype=np.uint8), min_cells=int(min_cells),
                max_dropout=int(max_dropout), reach=int(reach), min_track=int(min_track))


def settings(c):
    return {n: c[n] for n in ("min_cells", "max_dropout", "reach", "min_track")}


# ------------------------------------------------------------------ the hand cases
#
# name -> dict(classes, frames, settings..., want, want1).  `frames`: per frame the list entries, at most two.  `want` holds
# for every k >= 2 (the lists padded with EMPTY), `want1` for k = 1 (the lists cut to entry 0; where it is missing the
# case has one entry a frame and `want` holds).  A want is per frame (pred, age, id, len) rows over the first two entries
# plus (track, flags_out); pred None is 0xFF, an id is written as its root (frame, entry) and stands for frame * k + entry,
# None is 0xFFFFFFFF.  Entries behind the second read the empty values.
_ = None
A, B = obj(5, 2, 2, 3, 3), obj(4, 6, 2, 7, 3)
WIDE = obj(9, 2, 2, 7, 3)
FAR = obj(1, 65534, 65534, 65534, 65534)
BLANK = (3, 7, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF)            # three cells and the "no blob" box

HAND = {
    # three frames, one object that moves two cells a frame: box n + 1 begins one cell behind box n's end
    "chain": dict(classes="M M M", frames=[[obj(4, 2, 2, 3, 3)], [obj(4, 4, 2, 5, 3)], [obj(4, 6, 2, 7, 3)]], reach=1, min_track=3,
                  want=[([_, _], [1, 0], [(0, 0), _], [3, 0], 3, 1), ([0, _], [2, 0], [(0, 0), _], [3, 0], 3, 1),
                        ([0, _], [3, 0], [(0, 0), _], [3, 0], 3, 1)]),
    # ... and the same chain with reach 0: nothing touches, three tracks of one frame
    "chain apart": dict(classes="M M M", frames=[[obj(4, 2, 2, 3, 3)], [obj(4, 4, 2, 5, 3)], [obj(4, 6, 2, 7, 3)]], reach=0, min_track=2,
                        want=[([_, _], [1, 0], [(0, 0), _], [1, 0], 1, 0), ([_, _], [1, 0], [(1, 0), _], [1, 0], 1, 0),
                              ([_, _], [1, 0], [(2, 0), _], [1, 0], 1, 0)]),
    # one object falls into two: both halves continue entry 0
    "split": dict(classes="M M", frames=[[obj(6, 4, 4, 6, 5)], [obj(3, 3, 4, 4, 5), obj(3, 6, 4, 7, 5)]], reach=0, min_track=2,
                  want=[([_, _], [1, 0], [(0, 0), _], [2, 0], 2, 1), ([0, 0], [2, 2], [(0, 0), (0, 0)], [2, 2], 2, 1)],
                  want1=[([_], [1], [(0, 0)], [2], 2, 1), ([0], [2], [(0, 0)], [2], 2, 1)]),
    # two objects become one: it is linked to both and follows the lower rank; entry 1's track ends after one frame
    "merge": dict(classes="M M", frames=[[A, B], [WIDE]], reach=0, min_track=2,
                  want=[([_, _], [1, 1], [(0, 0), (0, 1)], [2, 1], 2, 1), ([0, _], [2, 0], [(0, 0), _], [2, 0], 2, 1)],
                  want1=[([_], [1], [(0, 0)], [2], 2, 1), ([0], [2], [(0, 0)], [2], 2, 1)]),
    # the same, but the lower rank has 4 cells and min_cells is 5 (an unsorted list is legal): it is absent, entry 1 is followed
    "merge absent": dict(classes="M M", frames=[[obj(4, 2, 2, 3, 3), obj(6, 6, 2, 7, 3)], [WIDE]], reach=0, min_cells=5, min_track=2,
                         want=[([_, _], [0, 1], [_, (0, 1)], [0, 2], 2, 1), ([1, _], [2, 0], [(0, 1), _], [2, 0], 2, 1)],
                         want1=[([_], [0], [_], [0], 0, 0), ([_], [1], [(1, 0)], [1], 1, 0)]),
    # entries that have cells but the all-0xFFFF box are present and link to nothing, whatever the reach
    "no box": dict(classes="M M", frames=[[BLANK], [BLANK]], reach=65535, min_track=1,
                   want=[([_, _], [1, 0], [(0, 0), _], [1, 0], 1, 1), ([_, _], [1, 0], [(1, 0), _], [1, 0], 1, 1)]),
    # bounds at 65534: 65534 <= 65534 + 65535 needs more than 16 bits; 0 + 65535 reaches 65534 ...
    "reach wide": dict(classes="M M M", frames=[[FAR], [FAR], [obj(1, 0, 0, 0, 0)]], reach=65535, min_track=3,
                       want=[([_, _], [1, 0], [(0, 0), _], [3, 0], 3, 1), ([0, _], [2, 0], [(0, 0), _], [3, 0], 3, 1),
                             ([0, _], [3, 0], [(0, 0), _], [3, 0], 3, 1)]),
    # ... and 0 + 65533 does not
    "reach short": dict(classes="M M", frames=[[obj(1, 0, 0, 0, 0)], [FAR]], reach=65533, min_track=2,
                        want=[([_, _], [1, 0], [(0, 0), _], [1, 0], 1, 0), ([_, _], [1, 0], [(1, 0), _], [1, 0], 1, 0)]),
    # reach 0: boxes that share a cell are linked, neighbours are not
    "reach 0": dict(classes="M M M", frames=[[FAR], [obj(2, 65533, 65534, 65534, 65534)], [obj(1, 65532, 65534, 65532, 65534)]], reach=0,
                    min_track=2,
                    want=[([_, _], [1, 0], [(0, 0), _], [2, 0], 2, 1), ([0, _], [2, 0], [(0, 0), _], [2, 0], 2, 1),
                          ([_, _], [1, 0], [(2, 0), _], [1, 0], 1, 0)]),
    # two quiet frames are bridged at max_dropout 2 ...
    "dropout at limit": dict(classes="M Q Q M", frames=[[A], [], [], [A]], max_dropout=2, min_track=2,
                             want=[([_, _], [1, 0], [(0, 0), _], [2, 0], 2, 1), ([_, _], [0, 0], [_, _], [0, 0], 0, 0),
                                   ([_, _], [0, 0], [_, _], [0, 0], 0, 0), ([0, _], [2, 0], [(0, 0), _], [2, 0], 2, 1)]),
    # ... three are not (the lists of quiet frames are never looked at)
    "dropout past limit": dict(classes="M Q Q Q M", frames=[[A], [A], [A], [A], [A]], max_dropout=2, min_track=2,
                               want=[([_, _], [1, 0], [(0, 0), _], [1, 0], 1, 0)] + [([_, _], [0, 0], [_, _], [0, 0], 0, 0)] * 3 +
                                    [([_, _], [1, 0], [(4, 0), _], [1, 0], 1, 0)]),
    # a key frame is transparent: it is no dropout
    "key frame": dict(classes="M T M", frames=[[A], [A], [A]], max_dropout=0, min_track=2,
                      want=[([_, _], [1, 0], [(0, 0), _], [2, 0], 2, 1), ([_, _], [0, 0], [_, _], [0, 0], 0, 0),
                            ([0, _], [2, 0], [(0, 0), _], [2, 0], 2, 1)]),
    # a motion frame with an empty list is p(f) of the next one and offers it nothing: track 0, then a new root
    "empty list": dict(classes="M M M", frames=[[A], [], [A]], min_track=1,
                       want=[([_, _], [1, 0], [(0, 0), _], [1, 0], 1, 1), ([_, _], [0, 0], [_, _], [0, 0], 0, 0),
                             ([_, _], [1, 0], [(2, 0), _], [1, 0], 1, 1)]),
}


def hand_case(name, k):
    """(case, want) of a hand case at k entries a frame; want: the six arrays."""
    h = HAND[name]
    fl, sd = pi.classes(h["classes"])
    c = case(fl, lists_of(h["frames"], k), sd=sd, **{n: h[n] for n in ("min_cells", "max_dropout", "reach", "min_track") if n in h})
    rows = h["want1"] if k == 1 and "want1" in h else h["want"]
    n = len(fl)
    want = {"pred": np.full((n, k), NO_PRED, dtype=np.uint8), "age": np.zeros((n, k), dtype=np.uint32),
            "id": np.full((n, k), NO_ID, dtype=np.uint32), "len": np.zeros((n, k), dtype=np.uint32),
            "track": np.zeros(n, dtype=np.uint32), "flags": np.zeros(n, dtype=np.uint8)}
    for f, (pr, ag, ids, ln, tr, fo) in enumerate(rows):
        for j in range(min(k, len(pr))):
            want["pred"][f, j] = NO_PRED if pr[j] is None else pr[j]
            want["age"][f, j] = ag[j]
            want["id"][f, j] = NO_ID if ids[j] is None else ids[j][0] * k + ids[j][1]
            want["len"][f, j] = ln[j]
        want["track"][f], want["flags"][f] = tr, fo
    return c, want


def embed(c, want, k, index=2, n_streams=4, seed=17):
    """The case's one stream as stream `index` of `n_streams` random ones: (case, slice, want of the slice — the ids moved
    by the stream's first frame times k, consequence D)."""
    rng = np.random.RandomState(seed)
    parts = []
    for s in range(n_streams):
        if s == index:
            parts.append((c["flags"], np.ones(len(c["flags"]), dtype=np.uint8) if c["sd"] is None else c["sd"], c["lists"]))
        else:
            parts.append(random_stream(rng, int(rng.randint(0, 30)), k))
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    e = dict(c, flags=np.concatenate([p[0] for p in parts]), sd=np.concatenate([p[1] for p in parts]),
             lists=np.concatenate([p[2] for p in parts]), soff=soff)
    moved = dict(want)
    moved["id"] = np.where(want["id"] == NO_ID, NO_ID, want["id"] + np.uint32(int(soff[index]) * k)).astype(np.uint32)
    return e, slice(int(soff[index]), int(soff[index + 1])), moved


# ------------------------------------------------------------------ the random generator of both tiers

def random_lists(rng, n, k, grid=(120, 68), movers=4, shuffle=True):
    """OBJECT_DTYPE [n, k]: up to `movers` boxes wander over the grid, each shows in a frame with its own probability and
    a size that flickers between 0 and 9 cells; sometimes a box jumps, sometimes an entry carries cells and the no-blob
    box.  With `shuffle` the entries of a frame — the empty ones among them — stand in random order: an unsorted list."""
    gw, gh = grid
    out = np.empty((n, k), dtype=OBJ)
    out[...] = EMPTY
    pos = [(int(rng.randint(0, gw - 8)), int(rng.randint(0, gh - 6))) for _ in range(movers)]
    show = [float(rng.uniform(0.4, 1.0)) for _ in range(movers)]
    for f in range(n):
        entries = []
        for m in range(movers):
            x, y = pos[m]
            if rng.random_sample() < 0.05:
                x, y = int(rng.randint(0, gw - 8)), int(rng.randint(0, gh - 6))
            else:
                x = int(np.clip(x + rng.randint(-3, 4), 0, gw - 8))
                y = int(np.clip(y + rng.randint(-2, 3), 0, gh - 6))
            pos[m] = (x, y)
            if rng.random_sample() < show[m]:
                w, h = int(rng.randint(0, 6)), int(rng.randint(0, 4))
                e = obj(int(rng.randint(0, 10)), x, y, x + w, y + h)
                if rng.random_sample() < 0.04:
                    e = (e[0], e[1]) + EMPTY[2:]
                entries.append(e)
        entries = (entries + [EMPTY] * k)[:k]
        if shuffle:
            entries = [entries[i] for i in rng.permutation(k)]
        for j, e in enumerate(entries):
            out[f, j] = e
    return out


def random_stream(rng, n, k, density=None, key_every=None):
    density = float(rng.uniform(0.3, 0.95)) if density is None else density
    key_every = (int(rng.randint(2, 31)) if rng.random_sample() < 0.8 else 0) if key_every is None else key_every
    fl, sd, _ = pi.random_stream(rng, n, density, key_every, False)
    return fl, sd, random_lists(rng, n, k)


def random_case(seed, k=None, max_streams=4, max_len=300, with_sd=None):
    """Draw `seed`: 1 .. max_streams streams of 0 .. max_len frames with unsorted lists of k entries (drawn from 1 .. 16
    when not given) and settings from the ranges where they bite."""
    rng = np.random.RandomState(4000 + seed)
    k = int(rng.choice([1, 2, 3, 4, 7, 15, 16])) if k is None else k
    with_sd = bool(rng.randint(0, 2)) if with_sd is None else with_sd
    parts = [random_stream(rng, int(rng.randint(0, max_len + 1)), k) for _ in range(int(rng.randint(1, max_streams + 1)))]
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    flags = np.concatenate([p[0] for p in parts])
    flags = np.where(flags != 0, rng.choice([1, 1, 2, 255], size=len(flags)), 0).astype(np.uint8)
    return case(flags, np.concatenate([p[2] for p in parts]), soff, np.concatenate([p[1] for p in parts]) if with_sd else None,
                min_cells=int(rng.choice([0, 1, 2, 4])), max_dropout=int(rng.choice([0, 0, 1, 2, 5, NO_LIMIT])),
                reach=int(rng.choice([0, 1, 2, 5, 20])), min_track=int(rng.choice([0, 1, 2, 3, 5])))


def single_streams(c):
    """The case cut into one case per stream (consequence D)."""
    out = []
    for s in range(len(c["soff"]) - 1):
        sl = slice(int(c["soff"][s]), int(c["soff"][s + 1]))
        out.append((sl, dict(c, flags=c["flags"][sl], lists=c["lists"][sl], soff=np.array([0, sl.stop - sl.start], dtype=np.uint64),
                             sd=None if c["sd"] is None else c["sd"][sl])))
    return out


def persist_twin(c):
    """Consequence A: a persistence case (tests/persist_inputs.py) as a tracks case at k = 1 — the entry carries the
    frame's box, and cells 1 where the frame is flagged."""
    n = len(c["flags"])
    li = np.empty((n, 1), dtype=OBJ)
    li[...] = EMPTY
    box = c["box"] if c["box"] is not None else pi.boxes(np.tile([3, 3, 4, 4], (n, 1)))
    for name in ("x0", "y0", "x1", "y1"):
        li[name][:, 0] = box[name]
    li["cells"][:, 0] = (c["flags"] != 0).astype(np.uint32)
    li["first"][:, 0] = 0
    return case(c["flags"], li, c["soff"], c["sd"], min_cells=1, max_dropout=c["max_dropout"],
                reach=c["reach"] if c["box"] is not None else 65535, min_track=c["min_run"]), box


# ------------------------------------------------------------------ tile seams (GPU tier)

def steady(n, k, step=1):
    """All-M lists: entry 0 walks right `step` cells a frame in a box three cells wide, entry 1 (k >= 2) shows every
    third frame at a fixed place far away: one track through the whole stream and many short ones."""
    frames = []
    for f in range(n):
        x = f * step
        e = [obj(6, x, 10, x + 2, 12)]
        if f % 3 == 0:
            e.append(obj(2, 60000, 60, 60001, 61))
        frames.append(e)
    return lists_of(frames, k)


def seam_cases(T, k, group=16, wave=64):
    """name -> case, one stream each.  T: frames_per_tile."""
    out = {}
    for n in (T - 1, T, T + 1, 2 * T + 1):
        # every consecutive pair of frames is linked: a link on every group seam, every wave seam and every tile seam
        out[f"steady {n}"] = case(np.ones(n, dtype=np.uint8), steady(n, k), reach=1, min_track=T)
        # the same with a key frame every 30 and quiet frames sprinkled in: p(f) is up to three frames back
        fl = np.ones(n, dtype=np.uint8)
        sd = np.ones(n, dtype=np.uint8)
        fl[::30] = 0
        sd[::30] = 0
        fl[7::11] = 0
        out[f"gaps {n}"] = case(fl, steady(n, k), sd=sd, reach=2, max_dropout=1, min_track=5)
    # a whole tile of Q and T frames between p(f) and f
    n = 2 * T + 1
    fl = np.zeros(n, dtype=np.uint8)
    fl[[3, 4, T + 40, T + 41]] = 1
    sd = np.ones(n, dtype=np.uint8)
    sd[5:T + 40:2] = 0
    li = lists_of([[obj(4, 20, 20, 22, 22)]] * n, k)
    out["tile of quiet"] = case(fl, li, sd=sd, max_dropout=NO_LIMIT, min_track=4)
    out["tile of quiet, bounded"] = case(fl, li, sd=sd, max_dropout=T // 2 - 1, min_track=2)
    # a split on each seam: frame s - 1 holds one object, frame s two that both continue it (k = 1: the list is cut)
    for s in (group, wave, T, 2 * T):
        frames = [[obj(8, 30, 30, 35, 32)] if f < s else [obj(4, 30, 30, 32, 32), obj(4, 34, 30, 35, 32)] for f in range(2 * T + 1)]
        out[f"split@{s}"] = case(np.ones(2 * T + 1, dtype=np.uint8), lists_of(frames, k), reach=0, min_track=2)
    return out


# ------------------------------------------------------------------ streams (GPU tier)

def streams_case(T, k, head=3, tail=5, seed=9):
    """70 streams back to back — empty ones, one-frame ones, one of T + 1 frames — `head` frames in front of the first and
    `tail` behind the last, all flagged and listed: those must read the empty values whatever they hold."""
    rng = np.random.RandomState(seed)
    lens = [0, 1, 2, 16, T + 1, 0, 0, 1] + [int(v) for v in rng.randint(1, 40, size=62)]
    soff = (head + np.concatenate([[0], np.cumsum(lens)])).astype(np.uint64)
    n = int(soff[-1]) + tail
    fl, sd, li = random_stream(rng, n, k, 0.7, 7)
    fl[:head] = 1
    fl[n - tail:] = 1
    return case(fl, li, soff, sd, min_cells=2, max_dropout=1, reach=3, min_track=2), lens


# ------------------------------------------------------------------ consequence C (GPU tier)

def sweep_case(k=4, seed=3, length=400, fps=10.0):
    rng = np.random.RandomState(seed)
    parts = [random_stream(rng, length, k, d, 30) for d in (0.2, 0.5, 0.85)]
    soff = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    pts = np.concatenate([np.arange(len(p[0]), dtype=np.float64) / fps for p in parts])
    return case(np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts]), soff, np.concatenate([p[1] for p in parts]),
                min_cells=2, max_dropout=1, reach=2), pts


# ------------------------------------------------------------------ end to end: two movers and one flicker

E2E_FRAMES = 24
E2E_FLICKER = 9
E2E_GRID = (40, 24)


def e2e_cells(f):
    """The blocks (x, y, w, h) of active cells of frame f on a 40 x 24 grid; every cell of a block has an active
    neighbour, so every one is a centre.  A 3 x 3 block walks right one cell a frame from frame 2 on; a 2 x 2 block walks
    down one cell a frame from frame 6 to 17; in frame 9 a 2 x 2 block flickers in a corner."""
    blocks = []
    if f >= 2:
        blocks.append((3 + f, 4, 3, 3))
    if 6 <= f <= 17:
        blocks.append((30, f, 2, 2))
    if f == E2E_FLICKER:
        blocks.append((4, 18, 2, 2))
    return blocks


def e2e_batch():
    """(params, mv, frame_off, has_sd): E2E_FRAMES frames, frame 12 a key frame without side data."""
    import blobs_inputs as bi
    p = bi.grid(*E2E_GRID)
    frames = []
    for f in range(E2E_FRAMES):
        cells = [(x + dx, y + dy) for (x, y, w, h) in e2e_cells(f) for dx in range(w) for dy in range(h)]
        frames.append(None if f == 12 else bi.cells_frame(cells))
    mv, off, sd = bi.batch_of(frames, 11)
    return p, mv, off, sd
