"""Inputs of the merge seam tests (tests/test_merge_seams_host.py, tests/test_gpu_merge_seams.py): timestamp lists that
walk the one-workgroup merge (merge_one_stream, csrc/merge_kernels.hip) over several chunks of T = 1024 with something
happening at the chunk and wave seams.  Everything is built deterministically; the expected values come from the
oracle (oracle_binding.pool_and_merge), never from the GPU, and the oracle itself is held to restate() below.

All timestamps and constants are binary-exact (multiples of 0.25), so a gap exactly equal to MAX_GAP, which is NOT a
split (`c - p > gap`, src/pipeline.cpp:333), can be placed on purpose.

A case is a Case: pts float64 [F], flags uint8 [F] or None (every frame pools its pts), mp MergeParams."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import mvtrim_amd as m

T, W = 1024, 64
N = 3 * T + 5                                    # the length of a seam case unless its name says otherwise
P_LIST = (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)
VARIANTS = ("sorted", "shuffled", "reversed", "dups", "chunk_runs")
LADDER_SIZES = (1537, 2047, 2048, 2049, 3071, 3072, 3073, 4095)      # what the default switch gives the one workgroup
ABOVE_SIZES = (4096, 4097, 8193, 20000)                              # ... and what only MTGPU_MERGE_LARGE_MIN does
NAN = float("nan")
MT_ERR_INVALID = 1


class Case(NamedTuple):
    family: str                                  # "dups", "segments", "inversion", "flags"
    pts: np.ndarray
    flags: Optional[np.ndarray]
    mp: m.MergeParams


def pooled(c):
    """The timestamps phase A pools: the pts of the flagged frames, in frame order."""
    return c.pts if c.flags is None else c.pts[c.flags != 0]


# ------------------------------------------------------------------ what a list is, from numpy alone

def phase_b_bits(ts):
    """(out of order, adjacent duplicates): bits 1 and 2 of phase B's `cond` on the pooled list."""
    ts = np.asarray(ts, dtype=np.float64)
    return bool((ts[1:] < ts[:-1]).any()), bool((ts[1:] == ts[:-1]).any())


def dup_indices(ts):
    """Indices i of the pooled list with ts[i] == ts[i - 1]: what phase D drops once the list is sorted."""
    ts = np.asarray(ts, dtype=np.float64)
    return np.flatnonzero(ts[1:] == ts[:-1]) + 1


def start_indices(u, gap):
    """Indices of the segment starts in a sorted unique list (phase E's is_start)."""
    u = np.asarray(u, dtype=np.float64)
    return np.concatenate([[0], np.flatnonzero(u[1:] - u[:-1] > gap) + 1]) if len(u) else np.zeros(0, dtype=np.int64)


def comparator_trips(n):
    """Trips of block_bitonic_sort's `for (p = threadIdx.x; p < halfP; p += MB)` loops on a list of n."""
    lg = 0
    while (1 << lg) < n:
        lg += 1
    half = (1 << (lg - 1)) if lg else 0
    return -(-half // T)


# ------------------------------------------------------------------ the sequential restatement (src/pipeline.cpp:302-358, 387-388)

def restate(ts, mp, job):
    """sort, unique, gap merge, pad, clamp, in-order sum, savings, cut, full-copy segment: one element after the other in
    Python floats (IEEE binary64).  Returns (segments SEGMENT_DTYPE [K], result dict) as the oracle does."""
    u = []
    for v in sorted(float(x) for x in ts):                            # :302
        if not u or not (v == u[-1]):                                 # :303-304
            u.append(v)
    res = dict(n_timestamps=len(u), n_segments=0, time_removed=0.0, saved_pct=0.0, do_cut=-1, status=0)
    if not u:                                                         # :308-319
        return np.zeros(0, dtype=m.SEGMENT_DTYPE), res
    gap, pad, dur = mp.max_gap_sec, mp.padding_sec, mp.duration
    raw, start, last = [], u[0], u[0]                                 # :328-329
    for v in u[1:]:
        if v - last > gap:                                            # :332-333
            raw.append((start, last))
            start = v
        last = v
    raw.append((start, last))
    segs, out_dur = [], 0.0
    for s, e in raw:
        s, e = s - pad, e + pad                                       # :337-338 / :343-344
        s = s if 0.0 < s else 0.0
        e = dur if dur < e else e                                     # :351
        s = e if e < s else s                                         # :352
        out_dur += e - s                                              # :353
        segs.append((s, e))
    removed = dur - out_dur                                           # :355
    pct = removed / dur * 100.0 if dur > 0 else 0.0                   # :356
    cut = 1 if pct > mp.min_savings_pct else 0                        # :358
    if job and not cut:                                               # :387-388
        segs = [(0.0, dur)]
    res.update(n_segments=len(segs), time_removed=removed, saved_pct=pct, do_cut=cut)
    return np.array(segs, dtype=m.SEGMENT_DTYPE), res


# ------------------------------------------------------------------ ladder: plain lists at the sizes the kernel has not seen

def _unique_values(rng, n):
    """n distinct multiples of 0.25, ascending: clusters 8 s apart with up to 13 members 0.25 s apart, a quarter of the
    places taken.  Gaps inside a cluster lie on both sides of 0.25 and 1.0, gaps between clusters start AT 5.0."""
    q = np.sort(rng.choice(4 * n, size=n, replace=False)) if n else np.zeros(0, dtype=np.int64)
    return (q // 13) * 8.0 + (q % 13) * 0.25


def _variant(rng, n, variant):
    """A list of exactly n timestamps.  `dups` holds n - n // 3 distinct values, one of them three times."""
    if variant == "dups":
        u = n - n // 3
        v = _unique_values(rng, u)
        extra = v[rng.randint(0, max(u, 1), size=n - u)] if n - u else v[:0]
        extra[:2] = v[:1]
        return rng.permutation(np.concatenate([v, extra]))
    v = _unique_values(rng, n)
    if variant == "shuffled":
        return rng.permutation(v)
    if variant == "reversed":
        return v[::-1].copy()
    if variant == "chunk_runs":                  # pooled per-chunk results: sorted runs of about 700, in any order
        runs = np.array_split(v, max(1, n // 700))
        order = rng.permutation(len(runs))
        if (order == np.arange(len(runs))).all():
            order = order[::-1]
        return np.concatenate([runs[i] for i in order])
    assert variant == "sorted"
    return v


def nominal_duration(n):
    return 8.0 * (4 * n // 13 + 1)


@functools.lru_cache(maxsize=None)
def ladder(n, variant):
    ts = _variant(np.random.RandomState(1000 * VARIANTS.index(variant) + n), n, variant)
    assert len(ts) == n
    ts.setflags(write=False)
    return ts


def ladder_params(n):
    """The three settings of test_merge_random (tests/test_gpu_parity.py) on the ladder's own duration."""
    dur = nominal_duration(n)
    return (m.MergeParams(duration=dur, max_gap_sec=5.0, padding_sec=0.5, min_savings_pct=5.0),
            m.MergeParams(duration=dur * 0.5, max_gap_sec=0.25, padding_sec=2.0, min_savings_pct=5.0),
            m.MergeParams(duration=0.0, max_gap_sec=1.0, padding_sec=0.0, min_savings_pct=5.0))


# ------------------------------------------------------------------ seam cases

GAP, PAD = 1.0, 0.25
NEAR, EQUAL, FAR = 0.25, 1.0, 1.25               # a step inside a segment, a step of exactly MAX_GAP, a split


def _from_steps(steps):
    steps = np.asarray(steps, dtype=np.float64).copy()
    steps[0] = 0.0
    return 8.0 + np.cumsum(steps)


def _mp(ts):
    finite = ts[ts == ts]
    dur = float(finite.max()) if len(finite) else 64.0               # the last segment's end is clamped (:351), to a
                                                                      # length of 0.25: leaving it out of the sum shows
    return m.MergeParams(duration=dur, max_gap_sec=GAP, padding_sec=PAD, min_savings_pct=5.0)


def _case(family, pts, flags=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    return Case(family, pts, flags, _mp(pooled(Case(family, pts, flags, None))))


def _weekly(n=N):
    """Steps of a sorted unique list with a split in front of every seventh element: 7-element segments, so that a
    value that lands in the wrong place moves a segment boundary."""
    steps = np.full(n, NEAR)
    steps[7::7] = FAR
    return steps


@functools.lru_cache(maxsize=None)
def seam_cases():
    out = {}
    # ---- duplicates: sorted input, phase D alone
    for p in P_LIST:
        s = _weekly()
        s[p] = 0.0
        out[f"dup-pair@{p}"] = _case("dups", _from_steps(s))                      # ts[p - 1] == ts[p]
        s = _weekly()
        s[p - 1:p + 3] = 0.0
        out[f"dup-run5@{p}"] = _case("dups", _from_steps(s))                      # ts[p - 2 .. p + 2] equal
    s = _weekly()
    s[501] = 0.0
    out["dup-chunk0-only"] = _case("dups", _from_steps(s))                        # every later chunk writes one behind its reads
    s = _weekly()
    s[T + 300] = 0.0
    out["dup-chunk1-only"] = _case("dups", _from_steps(s))                        # chunk 0 writes itself back unchanged
    out["dup-all-equal"] = _case("dups", np.full(N, 8.0))
    s = _weekly()
    s[2:T + 2] = 0.0
    out["dup-run-T+1-from-1"] = _case("dups", _from_steps(s))                     # ts[1 .. T + 1] equal
    # ---- segment boundaries: sorted and unique input, phase E
    for p in P_LIST:
        for name, step in (("split", FAR), ("nosplit", EQUAL)):
            s = np.full(N, NEAR)
            s[p] = step
            out[f"{name}@{p}"] = _case("segments", _from_steps(s))
    s = np.full(N, NEAR)
    s[W::W] = FAR
    out["split-every-wave-seam"] = _case("segments", _from_steps(s))
    s = np.full(N, NEAR)
    s[500] = s[2 * T + 300] = FAR
    out["span-chunk1"] = _case("segments", _from_steps(s))                        # [500, 2T + 300): no start in chunk 1
    s = np.full(N, NEAR)
    s[T - 1] = s[2 * T + 1] = FAR
    out["span-chunk1-tight"] = _case("segments", _from_steps(s))                  # [T - 1, 2T]: last lane to first lane
    for n, label in ((T, "T"), (T + 1, "T+1"), (N, "3T+5")):
        out[f"all-own-M={label}"] = _case("segments", _from_steps(np.full(n, FAR)))
    for k, label in ((T, "T"), (T + 1, "T+1")):
        s = np.full(N, NEAR)
        s[3::3][:k - 1] = FAR
        out[f"K={label}"] = _case("segments", _from_steps(s))
    # ---- one inversion: phase B sets the out-of-order bit, phase C sorts, nothing for phase D.  The two swapped
    # elements end one segment and start the next, so the answer depends on their order (left unsorted, K grows by one)
    base = _from_steps(_weekly())
    for p in P_LIST + (N - 1,):
        s = _weekly()
        s[p] = FAR
        v = _from_steps(s)
        v[[p - 1, p]] = v[[p, p - 1]]
        out["swap-last-two" if p == N - 1 else f"swap@{p}"] = _case("inversion", v)
    out["first-to-end"] = _case("inversion", np.concatenate([base[1:], base[:1]]))
    # ---- flags: the stream entry only
    out["flag-bytes"] = _case("flags", base, np.resize(np.array([0, 1, 2, 255, 0, 0, 1], dtype=np.uint8), N))
    out["flags-none"] = _case("flags", base, np.zeros(N, dtype=np.uint8))
    for p in P_LIST:
        f = np.zeros(N, dtype=np.uint8)
        f[p] = 1
        out[f"flag-one@{p}"] = _case("flags", base, f)
    f = np.resize(np.array([1, 1, 0, 7, 1], dtype=np.uint8), N)
    v = base.copy()
    quiet = [2, T - 2, T + 3, 2 * T + 4, N - 5]                                   # i % 5 == 2: unflagged, in every chunk
    assert not f[quiet].any()
    v[quiet] = NAN
    out["nan-unflagged"] = _case("flags", v, f)
    for p in P_LIST:
        v = base.copy()
        v[p] = NAN
        out[f"nan-flagged@{p}"] = _case("flags", v, np.ones(N, dtype=np.uint8))
    for c in out.values():
        c.pts.setflags(write=False)
        if c.flags is not None:
            c.flags.setflags(write=False)
    return out


N_SEAM_CASES = 16 + 20 + 8 + 15


def is_invalid(c):
    ts = pooled(c)
    return bool((ts != ts).any())


# two short streams that sit on either side of a seam case in a three-stream batch
NEIGHBOURS = (Case("short", np.array([9.0, 2.5, 2.0, 9.25, 1.0, 2.5]), None,
                   m.MergeParams(duration=12.0, max_gap_sec=1.0, padding_sec=0.25, min_savings_pct=5.0)),
              Case("short", np.array([3.0, 4.0, 5.25, 5.5, 40.0, 41.0, 41.25]), None,
                   m.MergeParams(duration=41.0, max_gap_sec=1.0, padding_sec=0.5, min_savings_pct=5.0)))


def three_streams(c):
    """The case as stream 1 of three, between NEIGHBOURS: (flags uint8 [F], pts [F], stream_off int64 [4], mps)."""
    parts = (NEIGHBOURS[0], c, NEIGHBOURS[1])
    flags = np.concatenate([np.ones(len(x.pts), dtype=np.uint8) if x.flags is None else x.flags for x in parts])
    pts = np.concatenate([x.pts for x in parts])
    off = np.concatenate([[0], np.cumsum([len(x.pts) for x in parts])]).astype(np.int64)
    return flags, pts, off, [x.mp for x in parts]


# ------------------------------------------------------------------ one device batch of streams

BATCH_LENS = (0, 1, T, T + 1, 2 * T + 1, 3 * T + 5, 4097, 20000)
LEVELS = (1, 2, 3, 5, 8, 13)
SIXTEEN = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 21, 1000)   # 0 counts as 1 (max(1, .)); 1000 keeps nothing
HEAD, TAIL = 3, 5


class Batch(NamedTuple):
    centres: np.ndarray          # int32 [F]; flags = centres >= 1
    flags: np.ndarray            # uint8 [F]
    pts: np.ndarray              # float64 [F]
    stream_off: np.ndarray       # int64 [S + 1]
    stream_off_over: np.ndarray  # the same with the last entry 1000 past F
    mps: tuple


@functools.lru_cache(maxsize=None)
def streams_batch():
    """Stream i: BATCH_LENS[i] frames, variant i mod 5, about 40 % of them flagged, its own MergeParams.  HEAD frames in
    front of the first stream hold NaN pts under set flags (no stream may read them), TAIL frames behind the last hold
    finite pts under set flags (the clamped overshoot of stream_off_over reads them).  The first six flagged frames
    (in a random order of the frames) of a stream carry the centre counts 1, 2, 3, 5, 8, 13, so LEVELS select strictly
    shrinking non-empty subsets of every stream that has six flagged frames; the one-frame stream carries 2."""
    rng = np.random.RandomState(30)
    cen = [np.full(HEAD, 99, dtype=np.int32)]
    pts = [np.full(HEAD, NAN)]
    mps = []
    for i, n in enumerate(BATCH_LENS):
        pts.append(_variant(rng, n, VARIANTS[i % 5]))
        c = np.zeros(n, dtype=np.int32)
        on = rng.permutation(n)[:int(round(0.4 * n))] if n > 1 else np.arange(n)
        c[on] = rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 6, 8, 10, 13, 20], size=len(on))
        if len(on) >= 6:
            c[on[:6]] = LEVELS
        elif n == 1:
            c[:] = 2
        cen.append(c)
        mps.append(m.MergeParams(duration=nominal_duration(n) * (0.5 if i % 4 == 2 else 1.0), max_gap_sec=5.0 if i % 2 else 1.0,
                                 padding_sec=0.25 * (i % 3), min_savings_pct=99.5 if i % 2 else 5.0))
    cen.append(np.full(TAIL, 99, dtype=np.int32))
    pts.append(1.0e6 + 16.0 * np.arange(TAIL))
    cen, pts = np.concatenate(cen), np.concatenate(pts)
    off = (HEAD + np.concatenate([[0], np.cumsum(BATCH_LENS)])).astype(np.int64)
    over = off.copy()
    over[-1] = len(pts) + 1000
    out = Batch(cen, (cen >= 1).astype(np.uint8), pts, off, over, tuple(mps))
    for a in out[:5]:
        a.setflags(write=False)
    return out


def sixteen_levels():
    """The same batch for 16 levels, the ABI's maximum (MT_SWEEP_MAX_LEVELS)."""
    return streams_batch(), SIXTEEN


def level_timestamps(b, i, need, off=None):
    """What stream i pools at one level: the pts of its frames with centres >= max(1, need), stream_off clamped to F."""
    off = b.stream_off if off is None else off
    lo, hi = min(int(off[i]), len(b.pts)), min(int(off[i + 1]), len(b.pts))
    return b.pts[lo:hi][b.centres[lo:hi] >= max(1, need)]


# ------------------------------------------------------------------ expected values (the oracle), computed once

def _oracle(ts, mp, job):
    import oracle_binding as ob
    if (np.asarray(ts) != np.asarray(ts)).any():
        return None                              # MT_ERR_INVALID: nothing of a NaN list is reported
    return ob.pool_and_merge(ts, mp, job)


@functools.lru_cache(maxsize=None)
def want_ladder(n, variant, job):
    return tuple(_oracle(ladder(n, variant), mp, job) for mp in ladder_params(n))


@functools.lru_cache(maxsize=None)
def want_seam(name, job):
    return _oracle(pooled(seam_cases()[name]), seam_cases()[name].mp, job)


@functools.lru_cache(maxsize=None)
def want_neighbours(job):
    return tuple(_oracle(x.pts, x.mp, job) for x in NEIGHBOURS)


@functools.lru_cache(maxsize=None)
def want_batch(levels, job, over=False):
    """[level][stream] -> (segments, result) of streams_batch()."""
    b = streams_batch()
    off = b.stream_off_over if over else b.stream_off
    return tuple(tuple(_oracle(level_timestamps(b, i, need, off), b.mps[i], job) for i in range(len(BATCH_LENS)))
                 for need in levels)


def all_expected_values():
    """Every expected value tests/test_gpu_merge_seams.py asks for (the host tier measures what they cost)."""
    for job in (False, True):
        for n in LADDER_SIZES + ABOVE_SIZES:
            for v in VARIANTS:
                want_ladder(n, v, job)
        for name in seam_cases():
            want_seam(name, job)
        want_neighbours(job)
        want_batch(LEVELS, job)
        want_batch(LEVELS, job, True)
        want_batch(SIXTEEN, job)
