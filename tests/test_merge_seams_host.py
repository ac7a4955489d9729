"""CPU tier of the merge seam tests: the inputs of tests/merge_seam_inputs.py reach what their names claim (from numpy
alone: M, K, phase B's bits, where duplicates and splits sit relative to the chunk seams of T = 1024 and the wave seams
of 64), and the oracle equals the sequential restatement of src/pipeline.cpp:302-358, 387-388 on every one of them,
bit for bit, with and without job semantics."""
import time

import numpy as np
import pytest

import merge_seam_inputs as mi
import oracle_binding as ob
from merge_seam_inputs import LADDER_SIZES, ABOVE_SIZES, N, P_LIST, T, VARIANTS, W

CASES = mi.seam_cases()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def unique_sorted(ts):
    return np.unique(np.asarray(ts, dtype=np.float64))


def m_and_k(ts, mp):
    """(M, K) of a finite list: distinct values, and segments of the gap merge."""
    u = unique_sorted(ts)
    return len(u), len(mi.start_indices(u, mp.max_gap_sec))


def chunk_of(i):
    return int(i) // T


def assert_oracle_is_the_restatement(ts, mp, what):
    for job in (False, True):
        wseg, wres = mi.restate(ts, mp, job)
        oseg, ores = ob.pool_and_merge(ts, mp, job)
        assert {k: ores[k] for k in ("n_timestamps", "n_segments", "do_cut", "status")} == \
            {k: wres[k] for k in ("n_timestamps", "n_segments", "do_cut", "status")}, (what, job)
        assert bits([ores["time_removed"], ores["saved_pct"]]).tolist() == bits([wres["time_removed"], wres["saved_pct"]]).tolist(), (what, job)
        assert np.array_equal(bits(oseg["start"]), bits(wseg["start"])) and np.array_equal(bits(oseg["end"]), bits(wseg["end"])), (what, job)


# ------------------------------------------------------------------ ladder

def test_ladder_sizes_and_bits():
    assert LADDER_SIZES == (1537, 2047, 2048, 2049, 3071, 3072, 3073, 4095) and ABOVE_SIZES == (4096, 4097, 8193, 20000)
    assert [mi.comparator_trips(n) for n in (1025, 2048, 2049, 4095, 4096, 4097, 8193, 20000)] == [1, 1, 2, 2, 2, 4, 8, 16]
    for n in LADDER_SIZES + ABOVE_SIZES:
        for v in VARIANTS:
            ts = mi.ladder(n, v)
            assert len(ts) == n and ts.dtype == np.float64 and np.array_equal(ts * 4.0, np.round(ts * 4.0))
            disorder, dups = mi.phase_b_bits(ts)
            assert disorder == (v != "sorted"), (n, v)        # every variant but `sorted` sets the out-of-order bit
            M = len(unique_sorted(ts))
            assert M == (n - n // 3 if v == "dups" else n), (n, v)
            if v != "dups":
                assert not dups
            else:
                vals, cnt = np.unique(ts, return_counts=True)
                assert cnt.max() >= 3 and (cnt == 1).any()
            if v != "sorted" and n >= 2049:
                assert len(ts) >= 2049 and mi.comparator_trips(len(ts)) >= 2       # the sort sees the POOLED list
            if v == "chunk_runs":
                runs = np.flatnonzero(ts[1:] < ts[:-1])
                assert 1 <= len(runs) <= max(1, n // 700) - 1         # runs that follow in order join up
            # gaps on both sides of every MAX_GAP of ladder_params, and gaps exactly equal to it
            g = np.diff(unique_sorted(ts))
            for mp in mi.ladder_params(n):
                assert (g > mp.max_gap_sec).any() and (g < mp.max_gap_sec).any() or mp.max_gap_sec == 0.25
                assert (g == mp.max_gap_sec).any(), (n, v, mp.max_gap_sec)
    assert all(n < 4096 for n in LADDER_SIZES) and all(n >= 4096 for n in ABOVE_SIZES)


@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_is_the_restatement_on_the_ladder(variant):
    for n in LADDER_SIZES + ABOVE_SIZES[:3]:
        for mp in mi.ladder_params(n):
            assert_oracle_is_the_restatement(mi.ladder(n, variant), mp, (n, variant, mp.max_gap_sec))


# ------------------------------------------------------------------ seam cases

def test_seam_case_list():
    assert len(CASES) == mi.N_SEAM_CASES == 59
    fam = [c.family for c in CASES.values()]
    assert [fam.count(f) for f in ("dups", "segments", "inversion", "flags")] == [16, 20, 8, 15]
    assert P_LIST == (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1) and N == 3 * T + 5
    for name, c in CASES.items():
        assert len(c.pts) == (N if "all-own-M=T" not in name else (T if name.endswith("=T") else T + 1)), name
        finite = c.pts[c.pts == c.pts]
        assert np.array_equal(finite * 4.0, np.round(finite * 4.0)), name
        assert (c.mp.max_gap_sec, c.mp.padding_sec) == (1.0, 0.25) and c.mp.duration * 4.0 == round(c.mp.duration * 4.0)
        assert (c.flags is None) == (c.family != "flags"), name
    # both answers of the cut decision occur, so job semantics is seen with and without the full-copy segment
    cuts = {mi.restate(mi.pooled(c), c.mp, False)[1]["do_cut"] for c in CASES.values() if not mi.is_invalid(c)}
    assert cuts == {-1, 0, 1}


def test_duplicate_cases_are_what_they_say():
    for name, c in CASES.items():
        if c.family != "dups":
            continue
        ts = mi.pooled(c)
        assert mi.phase_b_bits(ts) == (False, True), name                 # sorted, with adjacent duplicates: phase D alone
        d = mi.dup_indices(ts).tolist()
        M, K = m_and_k(ts, c.mp)
        assert M == N - len(d), name
        if name.startswith("dup-pair@"):
            assert d == [int(name.split("@")[1])]
        elif name.startswith("dup-run5@"):
            p = int(name.split("@")[1])
            assert d == [p - 1, p, p + 1, p + 2] and len(set(ts[p - 2:p + 3].tolist())) == 1
        elif name == "dup-chunk0-only":
            assert len(d) == 1 and chunk_of(d[0]) == 0 and 0 < d[0] < T - 1
        elif name == "dup-chunk1-only":
            assert len(d) == 1 and chunk_of(d[0]) == 1 and d[0] > T       # chunk 1's first predecessor, ts[T - 1], is untouched
        elif name == "dup-all-equal":
            assert M == 1 and K == 1 and len(d) == N - 1
        else:
            assert name == "dup-run-T+1-from-1" and d == list(range(2, T + 2)) and ts[0] < ts[1] and ts[T + 1] < ts[T + 2]
        if name != "dup-all-equal":
            assert K > 250                                                # 7-element segments: a misplaced value moves a boundary
    assert {n for n, c in CASES.items() if c.family == "dups"} >= {f"dup-pair@{p}" for p in P_LIST} | {f"dup-run5@{p}" for p in P_LIST}


def test_segment_cases_are_what_they_say():
    for name, c in CASES.items():
        if c.family != "segments":
            continue
        ts = mi.pooled(c)
        assert mi.phase_b_bits(ts) == (False, False), name                # sorted and unique: phases C and D are skipped
        M, K = m_and_k(ts, c.mp)
        st = mi.start_indices(ts, c.mp.max_gap_sec).tolist()
        assert M == len(ts) and K == len(st)
        seg = mi.restate(ts, c.mp, False)[0]
        assert (seg["end"] - seg["start"] > 0).all(), name                # the clamped last one too: every summand counts
        if K > T:
            assert (seg["end"][T:] - seg["start"][T:]).sum() > 0          # what phase F's later trips add
        if name.startswith("split@"):
            p = int(name.split("@")[1])
            assert st == [0, p] and ts[p] - ts[p - 1] > c.mp.max_gap_sec
            other = CASES[f"nosplit@{p}"]
            assert m_and_k(other.pts, other.mp) == (N, K - 1)             # the two differ in K by one
        elif name.startswith("nosplit@"):
            p = int(name.split("@")[1])
            assert st == [0] and ts[p] - ts[p - 1] == c.mp.max_gap_sec
        elif name == "split-every-wave-seam":
            assert st == list(range(0, N, W)) and K == 49
        elif name == "span-chunk1":
            assert K == 3 and chunk_of(st[1]) == 0 and chunk_of(st[2] - 1) == 2 and not [i for i in st if chunk_of(i) == 1]
        elif name == "span-chunk1-tight":
            assert st == [0, T - 1, 2 * T + 1] and not [i for i in st if chunk_of(i) == 1]      # starts on lane T - 1, ends on 2T
        elif name.startswith("all-own-M="):
            n = {"T": T, "T+1": T + 1, "3T+5": N}[name.split("=")[1]]
            assert K == M == n and -(-K // T) == {T: 1, T + 1: 2, N: 4}[n]                      # phase F's trips
        else:
            k = {"K=T": T, "K=T+1": T + 1}[name]
            assert K == k and M == N and chunk_of(st[-1]) >= 2                             # durs[] is written past the first chunk
    names = {n for n, c in CASES.items() if c.family == "segments"}
    assert names == {f"{a}@{p}" for a in ("split", "nosplit") for p in P_LIST} | {
        "split-every-wave-seam", "span-chunk1", "span-chunk1-tight", "all-own-M=T", "all-own-M=T+1", "all-own-M=3T+5", "K=T", "K=T+1"}


def test_inversion_cases_are_what_they_say():
    for name, c in CASES.items():
        if c.family != "inversion":
            continue
        ts = mi.pooled(c)
        assert mi.phase_b_bits(ts) == (True, False), name
        assert len(ts) == N >= 2049 and mi.comparator_trips(len(ts)) == 2
        down = (np.flatnonzero(ts[1:] < ts[:-1]) + 1).tolist()
        assert len(down) == 1                                             # ONE inversion
        if name.startswith("swap@"):
            assert down == [int(name.split("@")[1])]
        elif name == "swap-last-two":
            assert down == [N - 1]
        else:
            assert name == "first-to-end" and down == [N - 1] and ts[-1] < ts[0]
        M, K = m_and_k(ts, c.mp)
        assert M == N
        if name != "first-to-end":                                        # the pair ends one segment and starts the next:
            u, i = np.sort(ts), down[0]                                   # left unsorted, the list splits elsewhere
            assert u[i] - u[i - 1] > c.mp.max_gap_sec
            assert mi.start_indices(ts, c.mp.max_gap_sec).tolist() != mi.start_indices(u, c.mp.max_gap_sec).tolist()
    # the last step's comparator (2p, 2p + 1) that undoes swap@2049 and swap-last-two has p >= T: the sort's SECOND trip
    assert (2049 - 1) // 2 >= T and (N - 2) // 2 >= T


def test_flag_cases_are_what_they_say():
    for name, c in CASES.items():
        if c.family != "flags":
            continue
        ts = mi.pooled(c)
        if name == "flag-bytes":
            assert set(c.flags.tolist()) == {0, 1, 2, 255} and 0 < len(ts) < N and m_and_k(ts, c.mp)[0] == len(ts)
        elif name == "flags-none":
            assert len(ts) == 0 and mi.restate(ts, c.mp, True)[1]["do_cut"] == -1
        elif name.startswith("flag-one@"):
            assert len(ts) == 1 and ts[0] == c.pts[int(name.split("@")[1])]
        elif name == "nan-unflagged":
            bad = np.flatnonzero(c.pts != c.pts)
            assert len(bad) >= 3 and not c.flags[bad].any() and not mi.is_invalid(c) and T < len(ts) < N
            assert {chunk_of(i) for i in bad} == {0, 1, 2, 3}
        else:
            p = int(name.split("@")[1])
            assert np.flatnonzero(c.pts != c.pts).tolist() == [p] and c.flags[p] and mi.is_invalid(c)
            assert mi.want_seam(name, False) is None


def test_oracle_is_the_restatement_on_every_seam_case():
    n = 0
    for name, c in CASES.items():
        if mi.is_invalid(c):
            continue
        assert_oracle_is_the_restatement(mi.pooled(c), c.mp, name)
        n += 1
    assert n == 59 - 6
    for x in mi.NEIGHBOURS:
        assert_oracle_is_the_restatement(x.pts, x.mp, "neighbour")
        assert mi.phase_b_bits(x.pts)[0] or mi.phase_b_bits(x.pts) == (False, False)
    # the two neighbours by hand: [1, 2, 2.5] and [9, 9.25]; [3, 4] (a step of exactly MAX_GAP), [5.25, 5.5], [40, 41, 41.25]
    seg, res = mi.restate(mi.NEIGHBOURS[0].pts, mi.NEIGHBOURS[0].mp, False)
    assert seg.tolist() == [(0.75, 2.75), (8.75, 9.5)] and res["n_timestamps"] == 5
    seg, res = mi.restate(mi.NEIGHBOURS[1].pts, mi.NEIGHBOURS[1].mp, False)
    assert seg.tolist() == [(2.5, 4.5), (4.75, 6.0), (39.5, 41.0)] and res["n_timestamps"] == 7


# ------------------------------------------------------------------ the batch

def test_streams_batch_is_what_it_says():
    b = mi.streams_batch()
    S = len(mi.BATCH_LENS)
    assert mi.BATCH_LENS == (0, 1, T, T + 1, 2 * T + 1, 3 * T + 5, 4097, 20000) and mi.LEVELS == (1, 2, 3, 5, 8, 13)
    assert np.diff(b.stream_off).tolist() == list(mi.BATCH_LENS) and int(b.stream_off[0]) == mi.HEAD == 3
    F = len(b.pts)
    assert F == int(b.stream_off[-1]) + mi.TAIL == 3 + sum(mi.BATCH_LENS) + 5 and F < 40000 and max(mi.BATCH_LENS) <= 20000
    assert b.stream_off_over[:-1].tolist() == b.stream_off[:-1].tolist() and int(b.stream_off_over[-1]) == F + 1000
    assert np.isnan(b.pts[:3]).all() and b.flags[:3].all() and np.isfinite(b.pts[3:]).all() and b.flags[-5:].all()
    assert np.array_equal(b.flags, (b.centres >= 1).astype(np.uint8))
    inside = slice(int(b.stream_off[0]), int(b.stream_off[-1]))
    assert 0.38 < b.flags[inside].mean() < 0.42
    assert len({(p.duration, p.max_gap_sec, p.padding_sec, p.min_savings_pct) for p in b.mps}) == S
    big_k, cuts_of_big = 0, set()
    for i, n in enumerate(mi.BATCH_LENS):
        a, e = int(b.stream_off[i]), int(b.stream_off[i + 1])
        ts = b.pts[a:e]
        if n >= 2:
            assert mi.phase_b_bits(ts)[0] == (mi.VARIANTS[i % 5] != "sorted")
        sizes = [len(mi.level_timestamps(b, i, need)) for need in mi.LEVELS]
        if n >= T:                                   # every level's subset non-empty and strictly smaller than the one before
            assert all(x > y > 0 for x, y in zip(sizes, sizes[1:])) and sizes[-1] > 0, (i, sizes)
        elif n == 1:
            assert sizes == [1, 1, 0, 0, 0, 0]       # one frame cannot shrink six times: it leaves at level 3
        else:
            assert n == 0 and sizes == [0] * 6
        pooled = mi.level_timestamps(b, i, 1)
        if len(pooled):
            M, K = m_and_k(pooled, b.mps[i])
            if K > 64:
                big_k += 1
                cuts_of_big.add(mi.restate(pooled, b.mps[i], False)[1]["do_cut"])
            assert_oracle_is_the_restatement(pooled, b.mps[i], f"stream {i}")
    assert big_k >= 3 and cuts_of_big == {0, 1}      # the capacity test truncates, with and without the full-copy segment
    pooled7 = mi.level_timestamps(b, 7, 1)
    assert mi.comparator_trips(len(pooled7)) == 4 and len(pooled7) >= 4097
    # the clamped overshoot: the last stream reads the TAIL frames as well, at every level
    over = mi.level_timestamps(b, 7, 13, b.stream_off_over)
    assert len(over) == len(mi.level_timestamps(b, 7, 13)) + 5
    batch16, levels16 = mi.sixteen_levels()
    assert batch16 is b and len(levels16) == 16 and levels16[0] == 0 and len(mi.level_timestamps(b, 7, 1000)) == 0
    assert np.array_equal(mi.level_timestamps(b, 5, 0), mi.level_timestamps(b, 5, 1))


def test_expected_values_are_cheap():
    """All the oracle values of the GPU module; loosely bounded (measured: well under two seconds on one core)."""
    for f in (mi.want_ladder, mi.want_seam, mi.want_neighbours, mi.want_batch):
        f.cache_clear()
    t0 = time.process_time()
    mi.all_expected_values()
    cost = time.process_time() - t0
    print(f"expected values of tests/test_gpu_merge_seams.py: {cost:.2f} s of CPU time")
    assert cost < 10.0
