"""GPU tier (`-m gpu`): the one-workgroup merge (merge_one_stream of csrc/merge_kernels.hip, the body of
merge_streams_kernel and sweep_streams_kernel) on long, unordered and duplicated lists: several chunks of 1024, several
trips of the sort's comparator loops, duplicates, segment boundaries and inversions at the chunk and wave seams, more
than 1024 segments.  The inputs are tests/merge_seam_inputs.py, whose claims tests/test_merge_seams_host.py asserts on
the CPU.  The expected value is the oracle's pool_and_merge everywhere, and every comparison is on bit patterns.

mtgpu_merge_streams_device trusts stream_off (include/mtgpu.h: n_frames = d_stream_off[S]; it has no frame count to
clamp to), so the overshooting stream_off goes through mtgpu_sweep_streams_device only, which takes n_frames and clamps."""
import os

import numpy as np
import pytest

import mvtrim_amd as m

import merge_seam_inputs as mi
from merge_seam_inputs import ABOVE_SIZES, LADDER_SIZES, N, T, VARIANTS

pytestmark = pytest.mark.gpu

JOBS = [False, True]
S = len(mi.BATCH_LENS)
BIG_CAP = 8200                       # more than any stream of the batch pools


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def scanner(factory):
    return factory(m.ScanParams.from_config(1920, 1080))


def check(start, end, res, want, what, cap=None):
    """One stream's answer against the oracle's (segments, result), or against MT_ERR_INVALID where want is None.
    start / end: at least the first min(n_segments, cap) segments.  Returns the measured (M, K)."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: res[k].item())
    if want is None:
        assert (get("status"), get("n_timestamps"), get("n_segments"), get("do_cut")) == (mi.MT_ERR_INVALID, 0, 0, -1), what
        return 0, 0
    wseg, wres = want
    assert get("status") == 0, what
    for key in ("n_timestamps", "n_segments", "do_cut"):
        assert get(key) == wres[key], (what, key, get(key), wres[key])
    for key in ("time_removed", "saved_pct"):        # a NaN only has to be a NaN, as merge_case of test_gpu_parity.py allows
        g, w = get(key), wres[key]
        assert (g != g and w != w) or bits([g]).tolist() == bits([w]).tolist(), (what, key, g, w)
    k = int(wres["n_segments"]) if cap is None else min(int(wres["n_segments"]), cap)
    for got, exp, side in ((start, wseg["start"], "start"), (end, wseg["end"], "end")):
        bad = np.flatnonzero(bits(got[:k]) != bits(exp[:k]))
        assert bad.size == 0, (what, side, "first differing segment", int(bad[0]), float(got[bad[0]]), float(exp[bad[0]]))
    return int(wres["n_timestamps"]), int(wres["n_segments"])


def check_host(s, ts, mp, job, want, what):
    seg, res = s.merge_segments(ts, mp, job)
    assert len(seg) == res["n_segments"]
    return check(seg["start"], seg["end"], res, want, what)


def mp_tensor(mps):
    import torch
    return torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()


def filled(shape_bytes, byte):
    import torch
    return torch.full((shape_bytes,), byte, dtype=torch.uint8, device="cuda")


def junk_out(n_streams, cap, n_frames, ws_value, rows=None):
    """(segments [rows or n_streams, cap, 2] of 0x5A bytes, results [n_streams, 40] of 0x5A bytes, workspace [2F] of ws_value)."""
    import torch
    rows = n_streams if rows is None else rows
    seg = filled(rows * cap * 16, 0x5A).view(torch.float64).view(rows, cap, 2)
    res = filled(n_streams * 40, 0x5A).view(n_streams, 40)
    ws = torch.full((2 * n_frames,), ws_value, dtype=torch.float64, device="cuda")
    return seg, res, ws


def to_host(seg, res):
    import torch
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    return seg.cpu().numpy(), m.results_from_bytes(r.reshape(-1, 40)).reshape(r.shape[:-1])


# ------------------------------------------------------------------ a. the ladder on the default switch

@pytest.mark.parametrize("job", JOBS)
def test_ladder_on_the_default_switch(gpu_scanner_factory, job):
    """1537 .. 4095 timestamps x five variants x the three settings of test_merge_random through mtgpu_merge_segments on
    a context with the environment untouched: the largest lists the default switch (4096) gives the one workgroup."""
    assert "MTGPU_MERGE_LARGE_MIN" not in os.environ
    s = scanner(gpu_scanner_factory)
    for n in LADDER_SIZES:
        assert n < 4096
        for v in VARIANTS:
            ts = mi.ladder(n, v)
            for mp, want in zip(mi.ladder_params(n), mi.want_ladder(n, v, job)):
                M, _ = check_host(s, ts, mp, job, want, (n, v, mp.max_gap_sec))
                assert M == (n - n // 3 if v == "dups" else n)


# ------------------------------------------------------------------ b. above the switch, by the supported knob

@pytest.mark.parametrize("job", JOBS)
def test_ladder_above_the_switch(gpu_scanner_factory, monkeypatch, job):
    """4096 .. 20000 timestamps through the one-workgroup kernel (a context created under MTGPU_MERGE_LARGE_MIN = 10^8)
    and through the multi-workgroup path (a default context): byte-equal to each other and to the oracle."""
    monkeypatch.setenv("MTGPU_MERGE_LARGE_MIN", "100000000")
    one = scanner(gpu_scanner_factory)
    monkeypatch.delenv("MTGPU_MERGE_LARGE_MIN")
    many = scanner(gpu_scanner_factory)
    for n in ABOVE_SIZES:
        for v in VARIANTS:
            ts = mi.ladder(n, v)
            for mp, want in zip(mi.ladder_params(n), mi.want_ladder(n, v, job)):
                a, b = one.merge_segments(ts, mp, job), many.merge_segments(ts, mp, job)
                M, _ = check(a[0]["start"], a[0]["end"], a[1], want, ("one workgroup", n, v, mp.max_gap_sec))
                assert M == (n - n // 3 if v == "dups" else n) and len(a[0]) == a[1]["n_segments"]
                check(b[0]["start"], b[0]["end"], b[1], want, ("many workgroups", n, v, mp.max_gap_sec))
                assert a[0].tobytes() == b[0].tobytes() and bits([a[1]["time_removed"], a[1]["saved_pct"]]).tolist() == \
                    bits([b[1]["time_removed"], b[1]["saved_pct"]]).tolist()


# ------------------------------------------------------------------ c. the named seam cases

def measured_claims(name, M, K):
    """What a case's name says about M and K, on the measured values (without job semantics: K is then n_segments)."""
    if name.startswith("all-own-M="):
        n = {"T": T, "T+1": T + 1, "3T+5": N}[name.split("=")[1]]
        assert K == M == n, name
    elif name in ("K=T", "K=T+1"):
        assert (M, K) == (N, T if name == "K=T" else T + 1), name
    elif name.startswith("split@"):
        assert (M, K) == (N, 2), name
    elif name.startswith("nosplit@") or name == "dup-all-equal":
        assert K == 1, name
    elif name == "split-every-wave-seam":
        assert (M, K) == (N, 49), name
    elif name.startswith("span-chunk1"):
        assert (M, K) == (N, 3), name
    elif name.startswith("dup-pair@") or name in ("dup-chunk0-only", "dup-chunk1-only"):
        assert M == N - 1, name
    elif name.startswith("dup-run5@"):
        assert M == N - 4, name
    elif name == "dup-run-T+1-from-1":
        assert M == N - T, name
    elif name.startswith("flag-one@"):
        assert (M, K) == (1, 1), name
    elif name == "flags-none":
        assert (M, K) == (0, 0), name
    elif mi.seam_cases()[name].family == "inversion":
        assert M == N, name


@pytest.mark.parametrize("job", JOBS)
def test_seam_cases(gpu_scanner_factory, job):
    """Every named case through mtgpu_merge_streams_device as the middle one of three streams (its two short neighbours
    exact as well), and every case without flags through mtgpu_merge_segments and mtgpu_merge_timestamps_device too."""
    import torch
    s = scanner(gpu_scanner_factory)
    cases = mi.seam_cases()
    assert len(cases) == mi.N_SEAM_CASES
    near = mi.want_neighbours(job)
    for name, c in cases.items():
        want = mi.want_seam(name, job)
        if c.family != "flags":
            M, K = check_host(s, c.pts, c.mp, job, want, (name, "host entry"))
            if not job:
                measured_claims(name, M, K)
        flags, pts, off, mps = mi.three_streams(c)
        cap = len(c.pts) + 1
        seg, res = s.merge_streams_device(torch.from_numpy(flags).cuda(), torch.from_numpy(pts).cuda(),
                                          torch.from_numpy(off).cuda(), mp_tensor(mps), job_semantics=job, seg_cap=cap)
        seg, res = to_host(seg, res)
        check(seg[0, :, 0], seg[0, :, 1], res[0], near[0], (name, "stream in front"))
        check(seg[2, :, 0], seg[2, :, 1], res[2], near[1], (name, "stream behind"))
        M, K = check(seg[1, :, 0], seg[1, :, 1], res[1], want, (name, "stream entry"))
        if not job:
            measured_claims(name, M, K)
        if c.family != "flags":
            seg1, res1 = s.merge_timestamps_device(torch.from_numpy(c.pts.copy()).cuda(), c.mp, job, seg_cap=cap)
            seg1, res1 = to_host(seg1, res1)
            check(seg1[:, 0], seg1[:, 1], res1.reshape(-1)[0], want, (name, "timestamps entry"))


# ------------------------------------------------------------------ d. the batch of streams

def batch_tensors(b, off=None):
    import torch
    return (torch.from_numpy(b.flags.copy()).cuda(), torch.from_numpy(b.pts.copy()).cuda(),
            torch.from_numpy((b.stream_off if off is None else off).copy()).cuda(), mp_tensor(b.mps))


def check_rows(seg, res, wants, what, cap=None):
    mk = []
    for i, want in enumerate(wants):
        mk.append(check(seg[i, :, 0], seg[i, :, 1], res[i], want, (what, "stream", i), cap))
    return mk


@pytest.mark.parametrize("job", JOBS)
def test_streams_batch(gpu_scanner_factory, job):
    """streams_batch() in one mtgpu_merge_streams_device call, every stream against the oracle on its flagged pts; then
    through the out= form twice, the workspace pre-filled with NaNs (0x7FF8...) and then with 1e300, segments and results
    with 0x5A: both runs byte-equal, so the kernel reads nothing stale from its workspace."""
    s = scanner(gpu_scanner_factory)
    b = mi.streams_batch()
    wants, plain = mi.want_batch((1,), job)[0], mi.want_batch((1,), False)[0]
    d_flags, d_pts, d_off, d_mp = batch_tensors(b)
    seg, res = s.merge_streams_device(d_flags, d_pts, d_off, d_mp, job_semantics=job, seg_cap=BIG_CAP)
    seg, res = to_host(seg, res)
    mk = check_rows(seg, res, wants, "fresh buffers")
    assert [x[0] for x in mk] == [len(np.unique(mi.level_timestamps(b, i, 1))) for i in range(S)]
    assert mk[7][0] >= 4097                                   # the sort's loops made four trips on the last stream
    runs = []
    for junk in (float("nan"), 1e300):
        out = junk_out(S, BIG_CAP, len(b.pts), junk)
        if junk != junk:
            assert out[2][:1].cpu().numpy().view(np.uint64)[0] == 0x7FF8000000000000
        got = s.merge_streams_device(d_flags, d_pts, d_off, d_mp, job_semantics=job, seg_cap=BIG_CAP, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        seg2, res2 = to_host(*got)
        check_rows(seg2, res2, wants, f"out= over {junk}")
        runs.append((seg2.tobytes(), res2.tobytes()))
        for i, want in enumerate(plain):                      # behind the segments a stream finds its row is as it was
            k = int(want[1]["n_segments"])
            assert (seg2[i, k:].view(np.uint8) == 0x5A).all(), i
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ e. fewer slots than segments

def test_capacity_smaller_than_the_segments(gpu_scanner_factory):
    """seg_cap = 64 on the batch: n_segments reports K, the first 64 segments are exact, nothing is written behind a
    stream's own segments or into the row behind the last stream, and under job semantics without a cut slot 0 holds the
    full-copy segment."""
    s = scanner(gpu_scanner_factory)
    b = mi.streams_batch()
    d_flags, d_pts, d_off, d_mp = batch_tensors(b)
    cap = 64
    truncated = {False: 0, True: 0}
    for job in JOBS:
        wants = mi.want_batch((1,), job)[0]
        plain = mi.want_batch((1,), False)[0]
        seg_all, res, ws = junk_out(S, cap, len(b.pts), 1e300, rows=S + 1)
        got = s.merge_streams_device(d_flags, d_pts, d_off, d_mp, job_semantics=job, seg_cap=cap, out=(seg_all[:S], res, ws))
        seg, res = to_host(seg_all, got[1])
        assert (seg[S].view(np.uint8) == 0x5A).all()          # the row behind the last stream
        for i, want in enumerate(wants):
            K = int(plain[i][1]["n_segments"])                # the segments the merge finds, whatever is reported
            full_copy = job and want[1]["do_cut"] == 0
            M, k_got = check(seg[i, :, 0], seg[i, :, 1], res[i], want, ("capacity", job, i), cap)
            if full_copy:
                assert k_got == 1 and seg[i, 0].tolist() == [0.0, b.mps[i].duration]
            else:
                assert k_got == K
                assert (seg[i, min(K, cap):].view(np.uint8) == 0x5A).all(), (job, i)     # K <= 64: the bytes behind stay
            if K > cap:
                truncated[job] += 1
                if not full_copy:
                    assert res[i]["n_segments"].item() == K > cap
    assert truncated[False] >= 3 and truncated[True] >= 3


# ------------------------------------------------------------------ f. the sweep against the oracle

def sweep(s, b, levels, job, off=None, cap=BIG_CAP):
    import torch
    _, d_pts, d_off, d_mp = batch_tensors(b, off)
    seg, res = s.sweep_streams_device(torch.from_numpy(b.centres.copy()).cuda(), d_pts, d_off, d_mp, list(levels),
                                      job_semantics=job, seg_cap=cap)
    return to_host(seg, res)


@pytest.mark.parametrize("job", JOBS)
def test_sweep_rows_against_the_oracle(gpu_scanner_factory, job):
    """mtgpu_sweep_streams_device on the batch's centre counts with the levels [1, 2, 3, 5, 8, 13]: every (level, stream)
    row against the ORACLE on that level's timestamps; each level alone is byte-equal to its row of the joint launch (a
    level's workspace slice overlaps no other's); and with a stream_off whose last entry lies 1000 past the frames,
    which the kernel clamps: the last stream then reads up to the last frame."""
    s = scanner(gpu_scanner_factory)
    b = mi.streams_batch()
    wants = mi.want_batch(mi.LEVELS, job)
    seg, res = sweep(s, b, mi.LEVELS, job)
    sizes = []
    for l, need in enumerate(mi.LEVELS):
        mk = check_rows(seg[l], res[l], wants[l], f"level {need}")
        sizes.append([x[0] for x in mk])
    for i, n in enumerate(mi.BATCH_LENS):                     # measured: strictly shrinking, never empty
        if n >= T:
            col = [row[i] for row in sizes]
            assert all(x > y > 0 for x, y in zip(col, col[1:])), (i, col)
    for l, need in enumerate(mi.LEVELS):
        seg1, res1 = sweep(s, b, [need], job)
        assert seg1[0].tobytes() == seg[l].tobytes() and res1[0].tobytes() == res[l].tobytes(), need
    wants_over = mi.want_batch(mi.LEVELS, job, True)
    seg, res = sweep(s, b, mi.LEVELS, job, off=b.stream_off_over)
    for l, need in enumerate(mi.LEVELS):
        mk = check_rows(seg[l], res[l], wants_over[l], f"clamped, level {need}")
        assert mk[7][0] == sizes[l][7] + mi.TAIL


def test_sweep_sixteen_levels(gpu_scanner_factory):
    """The ABI's maximum of 16 levels in one launch; level 0 counts as 1, level 1000 keeps no frame."""
    s = scanner(gpu_scanner_factory)
    b, levels = mi.sixteen_levels()
    wants = mi.want_batch(levels, False)
    seg, res = sweep(s, b, levels, False)
    for l, need in enumerate(levels):
        mk = check_rows(seg[l], res[l], wants[l], f"level {need} of 16")
        if need == 1000:
            assert [x[0] for x in mk] == [0] * S
    assert seg[0].tobytes() == seg[1].tobytes() and res[0].tobytes() == res[1].tobytes()


# ------------------------------------------------------------------ g. a NaN stays in its stream

def test_nan_stays_in_its_stream(gpu_scanner_factory):
    """A NaN pts at a flagged frame at a chunk seam: that stream answers MT_ERR_INVALID with nothing reported, its
    neighbours in the batch are exact; through the sweep, the level that keeps the NaN frame answers the same and the
    level that drops it is exact on the frames that remain."""
    import torch
    s = scanner(gpu_scanner_factory)
    cases = mi.seam_cases()
    for job in JOBS:
        near = mi.want_neighbours(job)
        for p in mi.P_LIST:
            c = cases[f"nan-flagged@{p}"]
            flags, pts, off, mps = mi.three_streams(c)
            cap = N + 1
            d_pts, d_off, d_mp = torch.from_numpy(pts).cuda(), torch.from_numpy(off).cuda(), mp_tensor(mps)
            seg, res = to_host(*s.merge_streams_device(torch.from_numpy(flags).cuda(), d_pts, d_off, d_mp, job_semantics=job, seg_cap=cap))
            check(seg[0, :, 0], seg[0, :, 1], res[0], near[0], (p, "in front"))
            check(seg[1, :, 0], seg[1, :, 1], res[1], None, (p, "the NaN stream"))
            check(seg[2, :, 0], seg[2, :, 1], res[2], near[1], (p, "behind"))
            centres = np.full(len(pts), 2, dtype=np.int32)
            centres[int(off[1]) + p] = 1                      # level 1 keeps the NaN frame, level 2 drops it
            seg, res = to_host(*s.sweep_streams_device(torch.from_numpy(centres).cuda(), d_pts, d_off, d_mp, [1, 2],
                                                       job_semantics=job, seg_cap=cap))
            import oracle_binding as ob
            rest = ob.pool_and_merge(np.delete(c.pts, p), c.mp, job)
            for l, middle in enumerate((None, rest)):
                check(seg[l, 0, :, 0], seg[l, 0, :, 1], res[l, 0], near[0], (p, l, "in front"))
                M, _ = check(seg[l, 1, :, 0], seg[l, 1, :, 1], res[l, 1], middle, (p, l, "the NaN stream"))
                check(seg[l, 2, :, 0], seg[l, 2, :, 1], res[l, 2], near[1], (p, l, "behind"))
                assert M == (N - 1 if l else 0)
