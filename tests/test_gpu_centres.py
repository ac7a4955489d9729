"""GPU tier (`-m gpu`): the per-frame centre counts (the reference's `clusters` counter, src/motion_scanner.cpp:272-294,
without its early return) and the one-scan CLUSTERS_NEEDED sweep, against the oracle's mto_check_frame_count, the
hand-derived "centres" of tests/golden/check_frame_hand_cases.json and the existing flag / merge entry points.
Every comparison is exact: integers, and bit patterns of doubles."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, synth

import oracle_binding as ob
from golden_cases import build_mvs, id_of, load_hand_cases
from scan_checks import device_centres, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def oracle_centres(p, mv, off, has_sd=None):
    """(flags, centres) of every frame from the oracle, frame by frame.  has_sd None: side data iff records."""
    off = np.asarray(off).astype(np.int64)
    n = len(off) - 1
    flags, centres = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    for f in range(n):
        a, b = int(off[f]), int(off[f + 1])
        sd = (b > a) if has_sd is None else bool(has_sd[f])
        r, c, _ = ob.check_frame(p, mv[a:b], sd, count_centres=True)
        flags[f], centres[f] = r, c
    return flags, centres


# ------------------------------------------------------------------ arguments

def test_arguments_are_checked_before_anything_is_launched(gpu_scanner_factory):
    import torch
    lib = m.load_library()
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    inv = _abi.MT_ERR_INVALID
    rec = torch.zeros(8 * 16 + 8, dtype=torch.uint8, device="cuda")
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device="cuda")
    flags = torch.full((2,), 9, dtype=torch.uint8, device="cuda")
    cen = torch.full((2,), -7, dtype=torch.int32, device="cuda")

    def err():
        return lib.mtgpu_last_error().decode()

    for rb in (0, 7, 16, 39, 41, -8):
        assert lib.mtgpu_scan_centres_device(s._ctx, rec.data_ptr(), rb, 8, off.data_ptr(), None, 2, flags.data_ptr(),
                                             cen.data_ptr(), None) == inv
        assert "rec_bytes" in err()
    assert lib.mtgpu_scan_centres_device(s._ctx, rec.data_ptr(), 8, 8, off.data_ptr(), None, 2, None, None, None) == inv
    assert "d_flags" in err() and "d_centres" in err()
    assert lib.mtgpu_scan_centres_device(s._ctx, rec.data_ptr() + 4, 8, 8, off.data_ptr(), None, 2, flags.data_ptr(),
                                         cen.data_ptr(), None) == inv
    assert "d_rec" in err() and "8-byte" in err()
    assert lib.mtgpu_scan_frames_centres(s._ctx, None, None, None, 2, None, None) == inv
    # the sweep: n_levels 0 and 17, levels NULL
    pts = torch.zeros(2, dtype=torch.float64, device="cuda")
    soff = torch.tensor([0, 2], dtype=torch.int64, device="cuda")
    mp = torch.from_numpy(m.MergeParams(duration=1.0).to_record().view(np.uint8).copy()).cuda()
    ws = torch.zeros(17 * 4, dtype=torch.float64, device="cuda")
    seg = torch.zeros((17, 1, 4, 2), dtype=torch.float64, device="cuda")
    res = torch.full((17, 1, 40), 0x5A, dtype=torch.uint8, device="cuda")
    lv = (C.c_int32 * 17)(*range(1, 18))

    def sweep(levels, n_levels):
        return lib.mtgpu_sweep_streams_device(s._ctx, cen.data_ptr(), pts.data_ptr(), soff.data_ptr(), 1, 2, mp.data_ptr(),
                                              levels, n_levels, 0, ws.data_ptr(), seg.data_ptr(), 4, res.data_ptr(), None)
    assert sweep(lv, 0) == inv and "n_levels" in err()
    assert sweep(lv, 17) == inv and "n_levels" in err()
    assert sweep(None, 3) == inv and "levels" in err()
    torch.cuda.synchronize()
    # nothing was launched: no output changed
    assert flags.cpu().tolist() == [9, 9] and cen.cpu().tolist() == [-7, -7]
    assert int((res.cpu() != 0x5A).sum()) == 0 and float(seg.abs().sum()) == 0.0


# ------------------------------------------------------------------ hand cases

@pytest.mark.parametrize("force_fb", [None, 2, 8, 108])
@pytest.mark.parametrize("name,kw,case", load_hand_cases()[1], ids=id_of)
def test_hand_case_centres(gpu_scanner_factory, name, kw, case, force_fb):
    """Every hand-derived case: centres == case["centres"], flag == case["expect"]; host entry point, device entry
    point on 40-byte and on compact records, every counter form."""
    p = m.ScanParams.from_config(**kw)
    s = gpu_scanner_factory(p, force_fb=force_fb)
    mv = build_mvs(case)
    sd = int(case.get("has_sd", 1))
    b = m.FrameBatch(mv, np.array([0, len(mv)], dtype=np.uint64), None, np.array([sd], dtype=np.uint8))
    flags, centres = s.count_centres(b)
    print(name, "centres", centres.tolist(), "flag", flags.tolist(), "want", case["centres"], case["expect"])
    assert centres.dtype == np.uint32 and centres.tolist() == [case["centres"]], name
    assert flags.tolist() == [case["expect"]], name
    for compact in (False, True):
        fl, ce = device_centres(s, b.mv, b.frame_off, b.has_sd, compact)
        assert ce.tolist() == [case["centres"]] and fl.tolist() == [case["expect"]], (name, compact)


def test_hand_cases_one_batch_sliced_and_unsliced(gpu_scanner_factory):
    g, cases = load_hand_cases()
    base = [(n, c) for n, kw, c in cases if kw == g["base"]]
    assert len(base) >= 15
    p = m.ScanParams.from_config(**g["base"])
    frames = [build_mvs(c) if int(c.get("has_sd", 1)) else None for _, c in base]
    want_c = [c["centres"] for _, c in base]
    want_f = [c["expect"] if int(c.get("has_sd", 1)) else 0 for _, c in base]
    assert len(set(want_c)) >= 3
    b = m.FrameBatch.from_frames(frames)
    for slices in (1, 4):
        s = gpu_scanner_factory(p)
        s.set_slices(slices)
        flags, centres = s.count_centres(b)
        assert centres.tolist() == want_c and flags.tolist() == want_f, slices
        for compact in (False, True):
            fl, ce = device_centres(s, b.mv, b.frame_off, b.has_sd, compact)
            assert ce.tolist() == want_c and fl.tolist() == want_f, (slices, compact)


# ------------------------------------------------------------------ the oracle, every plan class

PLAN_CASES = [(1920, 1080, dict(), None, 0), (1920, 1080, dict(vectors_needed=3), 4, 0),
              (1920, 1080, dict(vectors_needed=9), 108, 2), (3840, 2160, dict(), None, 0),
              (3840, 2160, dict(block_size=4, block_shift=2, vectors_needed=1), None, 4),
              (3840, 2160, dict(block_size=4, block_shift=2, vectors_needed=4), None, 0),     # row bands (spill queue)
              (3840, 2160, dict(block_size=4, block_shift=2, vectors_needed=1), 32, 0),       # many row bands
              (1000, 600, dict(block_size=1, block_shift=0, vectors_needed=2, vertical_mask=0.0), None, 0)]


def test_centres_match_the_oracle_on_every_plan_class(gpu_scanner_factory):
    """The eight parameter sets of test_compact_records_match_aos_everywhere (single tile, packed forms, row bands, many
    row bands, sliced), drawn in that test's order from one RandomState(99): centres frame by frame, both record
    layouts, has_sd given and None; the flags are those of the existing entry point on the same context."""
    rng = np.random.RandomState(99)
    for k, (w, h, kw, fb, slices) in enumerate(PLAN_CASES):
        p = ob.params_from_config(w, h, **kw)
        s = gpu_scanner_factory(m.ScanParams.from_config(w, h, **kw), force_fb=fb)
        if slices:
            s.set_slices(slices)
        mv, off, sd = synth.random_frames(rng, 20, 6000, w, h, hot=0.5)
        for has_sd in (sd, None):
            want_f, want_c = oracle_centres(p, mv, off, has_sd)
            if has_sd is not None:
                print("set", k, (w, h, kw, fb, slices), "oracle centres", want_c.tolist())
                assert len(set(want_c.tolist())) >= (8 if k < 7 else 4), (k, sorted(set(want_c.tolist())))
            flags, centres = s.count_centres(m.FrameBatch(mv, off, None, has_sd))
            assert np.array_equal(centres, want_c), (k, has_sd is None, s.plan, centres.tolist(), want_c.tolist())
            assert np.array_equal(flags, want_f) and np.array_equal(flags, s.check_frames(m.FrameBatch(mv, off, None, has_sd)))
            for compact in (False, True):
                fl, ce = device_centres(s, mv, off, has_sd, compact)
                assert np.array_equal(ce, want_c), (k, has_sd is None, compact, s.plan, ce.tolist(), want_c.tolist())
                assert np.array_equal(fl, want_f), (k, has_sd is None, compact)
                fl0, ce0 = device_centres(s, mv, off, has_sd, compact, want_flags=False)      # d_flags == NULL
                assert fl0 is None and np.array_equal(ce0, want_c), (k, compact)


def test_centres_with_vectors_needed_zero(gpu_scanner_factory):
    """VECTORS_NEEDED 0: every cell is active, so a frame with side data — with records or with none — has every
    analysed cell with x in [1, grid_w - 2] as a centre; a frame without side data has none."""
    kw = dict(vectors_needed=0, clusters_needed=3)
    p = ob.params_from_config(1920, 1080, **kw)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, **kw))
    rng = np.random.RandomState(5)
    mv, off, sd = synth.random_frames(rng, 6, 500, 1920, 1080, hot=0.5)
    frames = [mv[int(off[i]):int(off[i + 1])] for i in range(6)] + [mv[:0], None, mv[3:4]]
    b = m.FrameBatch.from_frames(frames)
    b.has_sd[:6] = 1
    want_f, want_c = oracle_centres(p, b.mv, b.frame_off, b.has_sd)
    every = (p.grid_w - 2) * (p.grid_h - 2 * p.vertical_margin)
    assert want_c[6] == every and want_c[7] == 0 and want_c[8] == every and every > 1000
    flags, centres = s.count_centres(b)
    assert np.array_equal(centres, want_c) and np.array_equal(flags, want_f)
    for compact in (False, True):
        fl, ce = device_centres(s, b.mv, b.frame_off, b.has_sd, compact)
        assert np.array_equal(ce, want_c) and np.array_equal(fl, want_f), compact


def test_centres_large_batch_two_kernel_plan_and_grouped_frames(gpu_scanner_factory):
    """More than 32 768 frames (the two-kernel work-list plan) of a few KB each (several frames per workgroup), every
    second frame without side data although it owns records: 48 distinct small frames tiled, the oracle run once per
    distinct frame."""
    p = ob.params_from_config(1920, 1080)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    rng = np.random.RandomState(31)
    mv, off, _ = synth.random_frames(rng, 96, 400, 1920, 1080, hot=0.5)
    sd_tile = (np.arange(96) % 2 == 0).astype(np.uint8)
    want_f, want_c = oracle_centres(p, mv, off, sd_tile)
    assert len(set(want_c.tolist())) >= 6 and not want_c[1::2].any(), sorted(set(want_c.tolist()))
    reps = 420                                                               # 40 320 frames
    raw = np.tile(np.ascontiguousarray(mv).view(np.uint8).reshape(-1, 40), (reps, 1))
    big = raw.reshape(-1).view(m.MV_DTYPE)
    counts = np.tile(np.diff(off.astype(np.int64)), reps)
    off_big = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sd_big = np.tile(sd_tile, reps)
    assert len(sd_big) > 32768 and len(big) == int(off_big[-1])
    flags, centres = s.count_centres(m.FrameBatch(big, off_big, None, sd_big))
    bad = np.flatnonzero(centres != np.tile(want_c, reps))
    assert bad.size == 0, (bad[:8], centres[bad[:8]], np.tile(want_c, reps)[bad[:8]])
    assert np.array_equal(flags, np.tile(want_f, reps))
    fl, ce = device_centres(s, big, off_big, sd_big, compact=True)
    assert np.array_equal(ce, np.tile(want_c, reps)) and np.array_equal(fl, np.tile(want_f, reps))


# ------------------------------------------------------------------ unchanged behaviour, host-memory destination

def _build_c(tmp_path, name):
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", name + ".c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_every_centres_buffer_is_respected(tmp_path):
    """tests/c/abi_centres_canaries.c: buffers at exactly their stated sizes with canaries on both sides; with
    d_flags == NULL only the counts are written; results in pinned host memory."""
    exe = _build_c(tmp_path, "abi_centres_canaries")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all centre-count buffers respected" in out.stdout


def test_flags_of_the_centres_call_equal_the_plain_call(gpu_scanner_factory):
    import torch
    spec = synth.spec_1080p(seed=3, sub=1)
    spec.events = synth.scripted_events(spec, 64)
    mv, off, pts, sd = synth.gen_stream(spec, 64)
    p = ob.params_from_config(1920, 1080, vectors_needed=1)
    s = gpu_scanner_factory(p)
    d_mv, d_off, d_sd = to_device(mv, off, sd, False)
    d_rec, _, _ = to_device(mv, off, sd, True)
    plain = s.check_frames_device(d_mv, d_off, d_sd)
    plain8 = s.check_frames_device_compact(d_rec, d_off, d_sd)
    f40, c40 = s.count_centres_device(d_mv, d_off, d_sd)
    f8, c8 = s.count_centres_device(d_rec, d_off, d_sd, compact=True)
    torch.cuda.synchronize()
    assert 0 < int(plain.sum()) < 64
    assert torch.equal(plain, f40) and torch.equal(plain8, f8) and torch.equal(plain, plain8) and torch.equal(c40, c8)
    for need in (0, 1, 2, 3, 50, 10 ** 6):
        got = s.flags_from_centres(c40, need).cpu().numpy()
        assert np.array_equal(got, (c40.cpu().numpy() >= max(1, need)).astype(np.uint8)), need
    assert torch.equal(s.flags_from_centres(c40, p.clusters_needed), plain)


def test_centres_into_pinned_host_memory(gpu_scanner_factory):
    """d_centres (and d_flags) in pinned host memory the driver allocated (torch's pin_memory = hipHostMalloc), each on
    lines of its own: the same counts, nothing else written.  (tests/c/abi_centres_canaries.c does the same through
    hipHostGetDevicePointer.)"""
    import torch
    p = ob.params_from_config(1920, 1080)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    rng = np.random.RandomState(77)
    mv, off, sd = synth.random_frames(rng, 40, 3000, 1920, 1080, hot=0.5)
    want_f, want_c = oracle_centres(p, mv, off, sd)
    assert len(set(want_c.tolist())) >= 8
    n = len(off) - 1
    host = torch.empty(4096, dtype=torch.uint8).pin_memory()
    assert host.data_ptr() % 128 == 0
    host.fill_(0xEE)
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    # centres at +0, flags at +2048
    _abi.check(m.load_library().mtgpu_scan_centres_device(
        s._ctx, d_rec.data_ptr(), 8, len(mv), d_off.data_ptr(), d_sd.data_ptr(), n, host.data_ptr() + 2048,
        host.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw = host.numpy()
    assert np.array_equal(raw[:4 * n].view(np.uint32), want_c) and np.array_equal(raw[2048:2048 + n], want_f)
    assert (raw[4 * n:2048] == 0xEE).all() and (raw[2048 + n:] == 0xEE).all()


# ------------------------------------------------------------------ the pipe

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8, m.LAYOUT_AOS40, m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY,
                                    m.LAYOUT_AOS40 | m.LAYOUT_ZERO_COPY])
def test_pipe_carries_centres(gpu_scanner_factory, layout):
    """The batch shapes of test_scan_pipe_layouts_and_oversize_frames (oversize frame, empty frame, frames without side
    data), every layout | LAYOUT_CENTRES: drain_centres() gives the oracle's counts in tag order; a pipe without the
    flag refuses mtgpu_batch_centres and drains as before."""
    spec = synth.spec_1080p(seed=17, sub=1)
    spec.events = synth.scripted_events(spec, 90)
    frames = [synth.gen_frame(spec, i) for i in range(90)]
    frames[7] = np.zeros(0, dtype=m.MV_DTYPE)
    frames[40] = synth.gen_frame(synth.spec_1080p(seed=18, sub=2), 5)
    p = ob.params_from_config(1920, 1080, vectors_needed=1)
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, vectors_needed=1))
    b = m.FrameBatch.from_frames(frames)
    want_f, want_c = oracle_centres(p, b.mv, b.frame_off, b.has_sd)
    assert len(set(want_c.tolist())) >= 4 and any(f is None for f in frames)
    lib = m.load_library()
    st = _abi.PipeStatsC()
    for (max_rec, max_fr, nbuf) in [(8160 * 5, 7, 2), (8160, 1, 1), (100, 4, 2), (8160 * 3 + 17, 1000, 4)]:
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout, centres=True)) as pipe:
            _abi.check(lib.mtgpu_pipe_get_stats(pipe._pipe, C.byref(st)))
            assert st.layout == layout | m.LAYOUT_CENTRES
            for i, f in enumerate(frames):
                pipe.feed(f, spec.pts_seconds(i), tag=i)
            out = pipe.drain_centres()
            assert [t for _, _, t, _ in out] == list(range(90))
            assert [c for _, _, _, c in out] == want_c.tolist(), (max_rec, max_fr, nbuf)
            assert [fl for _, fl, _, _ in out] == want_f.tolist(), (max_rec, max_fr, nbuf)
    # without the flag: the same flags as ever, no centres
    cp = C.c_void_p()
    with contextlib.closing(m.ScanPipe(s, 8160 * 5, 7, 2, layout=layout)) as pipe:
        _abi.check(lib.mtgpu_pipe_get_stats(pipe._pipe, C.byref(st)))
        assert st.layout == layout
        for i, f in enumerate(frames[:10]):
            pipe.feed(f, spec.pts_seconds(i), tag=i)
        pipe._submit()
        bh, n = C.c_void_p(), C.c_uint32()
        _abi.check(lib.mtgpu_pipe_collect(pipe._pipe, C.byref(bh), None, None, None, C.byref(n)))
        rc, msg = lib.mtgpu_batch_centres(bh, C.byref(cp)), lib.mtgpu_last_error().decode()
        _abi.check(lib.mtgpu_pipe_release(pipe._pipe, bh))
        pipe._inflight -= 1
        assert rc == _abi.MT_ERR_INVALID and not cp.value and "MT_LAYOUT_CENTRES" in msg
        with pytest.raises(m.MtgpuError):
            pipe.drain_centres()
        assert 0 < n.value < 10 and [t for _, _, t in pipe.drain()] == list(range(n.value, 10))   # the rest of those ten
        for i, f in enumerate(frames):
            pipe.feed(f, spec.pts_seconds(i), tag=i)
        out = pipe.drain()
        assert [fl for _, fl, _ in out] == want_f.tolist() and [t for _, _, t in out] == list(range(90))
    # a batch that has not been collected
    with contextlib.closing(m.ScanPipe(s, 8160, 4, 2, layout=layout, centres=True)) as pipe:
        h = C.c_void_p()
        _abi.check(lib.mtgpu_pipe_acquire(pipe._pipe, C.byref(h)))
        rc, msg = lib.mtgpu_batch_centres(h, C.byref(cp)), lib.mtgpu_last_error().decode()
        _abi.check(lib.mtgpu_pipe_release(pipe._pipe, h))
        assert rc == _abi.MT_ERR_INVALID and "collected" in msg


# ------------------------------------------------------------------ the sweep

@pytest.mark.parametrize("job", [False, True])
def test_sweep_is_bit_identical_to_a_scan_per_level(gpu_scanner_factory, job):
    """16 streams x 32 frames, levels [0, 1, 2, 4, 8, 16]: every level and stream of ONE sweep launch on ONE scan's
    counts equals, bit for bit, (a) mtgpu_merge_streams_device on mtgpu_flags_from_centres_device's flags, (b) a fresh
    context created with clusters_needed = level, scanned and merged the existing way, (c) the oracle's pool_and_merge
    on the oracle's flags for that level."""
    import torch
    from test_gpu_golden import _gen_streams
    S, F, CAP = 16, 32, 32
    LEVELS = [0, 1, 2, 4, 8, 16]
    streams = _gen_streams(S, F, seed0=4000)
    mv = np.zeros(sum(len(st[1][0]) for st in streams), dtype=m.MV_DTYPE)
    pos = 0
    for st in streams:
        mv[pos:pos + len(st[1][0])] = st[1][0]
        pos += len(st[1][0])
    counts = np.concatenate([np.diff(st[1][1].astype(np.int64)) for st in streams])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.concatenate([st[1][2] for st in streams])
    sd = np.concatenate([st[1][3] for st in streams])
    mps = [m.MergeParams(duration=F / 30.0, max_gap_sec=0.2, padding_sec=0.05, min_savings_pct=5.0) for _ in range(S)]
    p1 = ob.params_from_config(1920, 1080)
    _, want_c = oracle_centres(p1, mv, off, sd)
    want_flags = {lv: (want_c >= max(1, lv)).astype(np.uint8) for lv in LEVELS}
    for lv in LEVELS:                                  # the oracle's own flag at that CLUSTERS_NEEDED says the same
        assert np.array_equal(ob.scan_frames(ob.params_from_config(1920, 1080, clusters_needed=lv), mv, off.astype(np.uint64), sd,
                                             nthreads=8), want_flags[lv]), lv
    print("flagged per level", {lv: int(want_flags[lv].sum()) for lv in LEVELS}, "distinct centres", len(set(want_c.tolist())))
    assert len({want_flags[lv].tobytes() for lv in LEVELS}) >= 3

    d_mv = torch.from_numpy(mv.view(np.uint8).reshape(-1)).cuda()
    d_off, d_sd, d_pts = torch.from_numpy(off).cuda(), torch.from_numpy(sd).cuda(), torch.from_numpy(pts).cuda()
    soff = torch.from_numpy(np.arange(S + 1, dtype=np.int64) * F).cuda()
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))
    _, centres = s.count_centres_device(d_mv, d_off, d_sd)
    seg, res = s.sweep_streams_device(centres, d_pts, soff, d_mp, LEVELS, job_semantics=job, seg_cap=CAP)
    torch.cuda.synchronize()
    assert np.array_equal(centres.cpu().numpy().view(np.uint32), want_c)
    assert tuple(seg.shape) == (len(LEVELS), S, CAP, 2) and tuple(res.shape) == (len(LEVELS), S, 40)
    seg_h, res_h = seg.cpu().numpy(), res.cpu().numpy()
    for li, lv in enumerate(LEVELS):
        # (a) the existing merge on flags derived from the counts
        fl = s.flags_from_centres(centres, lv)
        seg_a, res_a = s.merge_streams_device(fl, d_pts, soff, d_mp, job_semantics=job, seg_cap=CAP)
        # (b) a fresh context with clusters_needed = level, the existing way end to end
        sb = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, clusters_needed=lv))
        fl_b = sb.check_frames_device(d_mv, d_off, d_sd)
        seg_b, res_b = sb.merge_streams_device(fl_b, d_pts, soff, d_mp, job_semantics=job, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(fl.cpu().numpy(), want_flags[lv]) and np.array_equal(fl_b.cpu().numpy(), want_flags[lv]), lv
        for name, sg, rs in (("a", seg_a, res_a), ("b", seg_b, res_b)):
            assert np.array_equal(bits(seg_h[li]), bits(sg.cpu().numpy())), (lv, name)
            assert np.array_equal(res_h[li], rs.cpu().numpy()), (lv, name)
        # (c) the oracle
        recs = m.results_from_bytes(res_h[li])
        for i in range(S):
            a, b = i * F, (i + 1) * F
            wseg, wres = ob.pool_and_merge(pts[a:b][want_flags[lv][a:b] != 0], mps[i], job)
            wrec = np.zeros(1, dtype=m.MERGE_RESULT_DTYPE)
            for k, v in wres.items():
                wrec[k] = v
            assert recs[i:i + 1].tobytes() == wrec.tobytes(), (lv, i, recs[i], wres)
            k = int(wres["n_segments"])
            assert np.array_equal(bits(seg_h[li, i, :k, 0]), bits(wseg["start"])), (lv, i)
            assert np.array_equal(bits(seg_h[li, i, :k, 1]), bits(wseg["end"])), (lv, i)


# ------------------------------------------------------------------ front end

def test_scan_file_sweep_and_centres(tmp_path):
    """mtgpu_scan_file --sweep 1,4,5 --centres on the hand-derived whole-video case (every frame with records has exactly
    4 centres): entry k is the tool's own output under CLUSTERS_NEEDED=k — levels 1 and 4 the known [[0, 3]], level 5 no
    motion at all; one [pts, n] pair per analysed frame; without the options the output has today's fields only."""
    from test_gpu_golden import _filter_golden_stream
    g, pl, frames, ticks, path = _filter_golden_stream(tmp_path)
    exe = os.path.join(os.path.dirname(m.LIB_PATH), "mtgpu_scan_file")
    env = dict(os.environ, CHUNK_DURATION_SEC=str(pl["chunk_sec"]), TARGET_FPS=str(pl["target_fps"]),
               MAX_GAP_SEC="5.0", PADDING_SEC="0.5", MIN_SAVINGS_PCT="5")
    for k in ("VECTORS_NEEDED", "CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)

    def run(args, **extra):
        out = subprocess.run([exe, path, "--threads", "2"] + args, check=True, capture_output=True, text=True,
                             env=dict(env, **extra), timeout=120).stdout
        return out, json.loads(out)

    text, plain = run([])
    assert list(plain) == ["input", "chunks", "threads", "frames_scanned", "motion_frames", "n_timestamps", "do_cut",
                           "time_removed", "saved_pct", "seek_us", "decode_us", "analyze_us", "init_us", "scan_wall_us",
                           "scan_work_us", "copy_us", "submit_us", "wait_us", "segments"]
    assert text.rstrip().endswith('"segments": [[0, 3]]}') and plain["segments"] == [[0.0, 3.0]]
    _, r = run(["--sweep", "1,4,5", "--centres"])
    assert {k: r[k] for k in ("segments", "do_cut", "saved_pct", "n_timestamps", "time_removed", "motion_frames", "frames_scanned")} == \
        {k: plain[k] for k in ("segments", "do_cut", "saved_pct", "n_timestamps", "time_removed", "motion_frames", "frames_scanned")}
    assert [e["clusters_needed"] for e in r["sweep"]] == [1, 4, 5]
    for e in r["sweep"]:
        _, own = run([], CLUSTERS_NEEDED=str(e["clusters_needed"]))
        for k in ("segments", "do_cut", "saved_pct", "n_timestamps"):
            assert e[k] == own[k], (e, own)
    assert r["sweep"][0]["segments"] == [[0.0, 3.0]] and r["sweep"][1]["segments"] == [[0.0, 3.0]]
    assert r["sweep"][2]["segments"] == [] and r["sweep"][2]["do_cut"] == -1 and r["sweep"][2]["n_timestamps"] == 0
    analysed = sorted({f for chunk in pl["per_chunk"] for f in chunk})
    assert r["centres"] == [[f / 32.0, 0 if f in pl["keyframes"] else 4] for f in analysed]
    assert len(r["centres"]) == r["frames_scanned"] and any(c[1] == 0 for c in r["centres"])
    _, only_c = run(["--centres"])
    assert only_c["centres"] == r["centres"] and "sweep" not in only_c


def test_plain_c_centres_example(tmp_path):
    """examples/centres_example.c: one scan, segments for three CLUSTERS_NEEDED values, from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "centres_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "centres_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "centres: frame 15 -> 2, frame 60 -> 6, frame 80 -> 0" in out.stdout
    assert "CLUSTERS_NEEDED 2: motion frames 30, segments 2" in out.stdout
    assert "CLUSTERS_NEEDED 4: motion frames 20, segments 1" in out.stdout and "CLUSTERS_NEEDED 8: motion frames 0, segments 0" in out.stdout


# ------------------------------------------------------------------ threads

def test_one_context_counts_centres_from_many_threads(gpu_scanner_factory):
    """test_one_context_entered_from_many_threads with the centre counts: eight threads on one context, each calling
    count_centres_device (40-byte and compact) on its own stream, the host entry point and a centres pipe."""
    import torch
    spec = synth.spec_1080p(seed=23, sub=1)
    spec.events = synth.scripted_events(spec, 90)
    p = ob.params_from_config(1920, 1080, vectors_needed=1)
    s = gpu_scanner_factory(p)
    errors, lock = [], threading.Lock()

    def worker(w):
        try:
            rng = np.random.default_rng(100 + w)
            frames = [synth.gen_frame(spec, int(i)) for i in rng.integers(0, 90, size=40)]
            b = m.FrameBatch.from_frames(frames)
            want_f, want_c = oracle_centres(p, b.mv, b.frame_off, b.has_sd)
            st = torch.cuda.Stream()
            d_mv, d_off, d_sd = to_device(b.mv, b.frame_off, b.has_sd, False)
            d_rec, _, _ = to_device(b.mv, b.frame_off, b.has_sd, True)
            torch.cuda.synchronize()
            for it in range(6):
                f0, c0 = s.count_centres(b)
                assert np.array_equal(c0, want_c) and np.array_equal(f0, want_f)
                f1, c1 = s.count_centres_device(d_mv, d_off, d_sd, stream=st.cuda_stream)
                f2, c2 = s.count_centres_device(d_rec, d_off, d_sd, compact=True, flags=False, stream=st.cuda_stream)
                pipe = m.ScanPipe(s, 8160 * 6, 16, 2, layout=(m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY) if it % 2 else m.LAYOUT_AOS40,
                                  centres=True)
                with contextlib.closing(pipe):
                    for i, f in enumerate(frames):
                        pipe.feed(f, float(i), tag=i)
                    out = pipe.drain_centres()
                assert [c for _, _, _, c in out] == want_c.tolist()
                st.synchronize()
                assert np.array_equal(c1.cpu().numpy().view(np.uint32), want_c) and np.array_equal(f1.cpu().numpy(), want_f)
                assert f2 is None and np.array_equal(c2.cpu().numpy().view(np.uint32), want_c)
        except BaseException as e:          # noqa: BLE001 - reported to the main thread
            with lock:
                errors.append((w, repr(e)))

    threads = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
