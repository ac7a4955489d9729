"""GPU tier (`-m gpu`): a keep mask carried through the pipe (include/mtgpu_pipe_zones.h; csrc/zones_kernels.hip, the
pipe form), the C++ host layer and mtgpu_scan_file.  Expected values: the oracle on the same frames with every record
removed whose destination cell is ignored (tests/pipe_zones_inputs.py; checked without a GPU by
tests/test_pipe_zones_host.py), counts derived by hand where a case says so, and mtgpu_scan_frames_zones on the same
frames as one stream."""
import contextlib
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import oracle_binding as ob
import pipe_zones_inputs as pz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC = m.LAYOUT_ZERO_COPY
LAYOUTS = [m.LAYOUT_COMPACT8, m.LAYOUT_AOS40, m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC]
LAYOUT_IDS = ["compact8", "aos40", "compact8-zero-copy", "aos40-zero-copy"]


def feed_all(pipe, frames, pts=None):
    for i, f in enumerate(frames):
        pipe.feed(f, float(i) if pts is None else pts[i], tag=i)


def run(pipe, frames, pts=None):
    """Feed, drain -> (flags, centres) lists in tag order (the pipe returns submission order: asserted equal)."""
    feed_all(pipe, frames, pts)
    out = pipe.drain_centres()
    assert [t for _, _, t, _ in out] == list(range(len(frames)))
    return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]


def zones_host_entry(s, p, frames, keep):
    """mtgpu_scan_frames_zones on the same frames as one stream."""
    fl, ce, _ = s.scan_zones(m.FrameBatch.from_frames(list(frames)), [0, len(frames)], zones.pack_keep(keep))
    return fl.tolist(), ce.tolist()


# ------------------------------------------------------------------ 1. layouts x batch shapes

@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_masked_pipe_in_every_layout_and_batch_shape(gpu_scanner_factory, layout):
    """The batch shapes of test_pipe_carries_centres (frames per batch 7 / 1 / 4 / all 90; the 100-record batch grows
    for every frame), 90 1080p frames, mask A: flags and counts in tag order are the oracle's on the filtered records
    and what mtgpu_scan_frames_zones returns."""
    p, frames, pts, keep_a, _, want = pz.hd_case()
    s = gpu_scanner_factory(p)
    want_f, want_c = want["a"][0].tolist(), want["a"][1].tolist()
    assert zones_host_entry(s, p, frames, keep_a) == (want_f, want_c)
    for (max_rec, max_fr, nbuf) in [(8160 * 5, 7, 2), (8160, 1, 1), (100, 4, 2), (8160 * 3 + 17, 1000, 4)]:
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout, centres=True)) as pipe:
            assert pipe.has_keep is False
            pipe.set_keep(keep_a)
            assert pipe.has_keep is True
            got_f, got_c = run(pipe, frames, pts)
            assert got_c == want_c, (max_rec, max_fr, nbuf)
            assert got_f == want_f, (max_rec, max_fr, nbuf)
    # a pipe without centre counts carries the same flags
    with contextlib.closing(m.ScanPipe(s, 8160 * 5, 7, 2, layout=layout)) as pipe:
        pipe.set_keep(zones.pack_keep(keep_a))                # packed words are taken as they are
        feed_all(pipe, frames, pts)
        out = pipe.drain()
        assert [fl for _, fl, _ in out] == want_f and [t for _, _, t in out] == list(range(90))


# ------------------------------------------------------------------ 2. all-ones mask, dropping the mask

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40], ids=["compact8-zero-copy", "aos40"])
def test_full_mask_and_no_mask_are_the_plain_scan(gpu_scanner_factory, layout):
    p, frames, pts, keep_a, _, want = pz.hd_case()
    s = gpu_scanner_factory(p)
    plain_f, plain_c = want["none"][0].tolist(), want["none"][1].tolist()
    with contextlib.closing(m.ScanPipe(s, 8160 * 5, 7, 2, layout=layout, centres=True)) as pipe:
        assert run(pipe, frames, pts) == (plain_f, plain_c) and not pipe.has_keep
        pipe.set_keep(np.ones((p.grid_h, p.grid_w), dtype=bool))
        assert pipe.has_keep and run(pipe, frames, pts) == (plain_f, plain_c)
        pipe.set_keep(keep_a)
        assert run(pipe, frames, pts) == (want["a"][0].tolist(), want["a"][1].tolist())
        pipe.set_keep(None)
        assert not pipe.has_keep and run(pipe, frames, pts) == (plain_f, plain_c)
        pipe.set_keep(None)                                    # dropping no mask is not an error
        assert not pipe.has_keep
        with pytest.raises(ValueError):
            pipe.set_keep(np.ones((p.grid_h, p.grid_w + 1), dtype=bool))
        assert not pipe.has_keep


# ------------------------------------------------------------------ 3. one pipe, two recordings

def test_one_pipe_two_recordings_and_busy(gpu_scanner_factory):
    p, frames, pts, keep_a, keep_b, want = pz.hd_case()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    exp = {k: (v[0].tolist(), v[1].tolist()) for k, v in want.items()}
    with contextlib.closing(m.ScanPipe(s, 8160 * 5, 7, 3, centres=True)) as pipe:
        pipe.set_keep(keep_a)
        assert run(pipe, frames, pts) == exp["a"]
        # a batch being filled: MT_ERR_BUSY, and the run that follows still uses mask A
        feed_all(pipe, frames[:3], pts)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(keep_b)
        assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value) and pipe.has_keep
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(None)
        assert e.value.code == _abi.MT_ERR_BUSY and pipe.has_keep
        for i in range(3, 90):
            pipe.feed(frames[i], pts[i], tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == exp["a"]
        # a batch in flight: the same
        feed_all(pipe, frames[:20], pts)                       # 7 + 7 submitted, 6 being filled
        pipe._submit()
        assert pipe._cur is None and pipe._inflight >= 1
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(keep_b)
        assert e.value.code == _abi.MT_ERR_BUSY and "in flight" in str(e.value) and pipe.has_keep
        for i in range(20, 90):
            pipe.feed(frames[i], pts[i], tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == exp["a"]
        # a batch that is collected but not yet released does not matter
        bh = C_void()
        _abi.check(lib.mtgpu_pipe_acquire(pipe._pipe, bh.ref))
        _abi.check(lib.mtgpu_pipe_submit(pipe._pipe, bh.ptr))
        got = C_void()
        _abi.check(lib.mtgpu_pipe_collect(pipe._pipe, got.ref, None, None, None, None))
        pipe.set_keep(keep_b)
        _abi.check(lib.mtgpu_pipe_release(pipe._pipe, got.ptr))
        assert run(pipe, frames, pts) == exp["b"]
        pipe.set_keep(None)
        assert run(pipe, frames, pts) == exp["none"]
    assert exp["a"] != exp["b"] != exp["none"]


class C_void:
    def __init__(self):
        import ctypes
        self.ptr = ctypes.c_void_p()
        self.ref = ctypes.byref(self.ptr)


# ------------------------------------------------------------------ 4. stale results in the pinned block

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
def test_no_stale_results_in_a_reused_pinned_block(gpu_scanner_factory, layout):
    """n_buffers = 1, zero-copy: batch 1 leaves flag 1 / count 2 for every frame in the pinned block; batch 2 goes into
    the same block — frames without side data (answered by the planning kernel) and frames whose motion the zone removes
    entirely (answered by the masked scan) — and must read 0 everywhere."""
    p, one, two, keep = pz.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 4096, 12, 1, layout=layout, centres=True)) as pipe:
        pipe.set_keep(keep)
        assert run(pipe, one) == ([1] * 12, [2] * 12)
        assert run(pipe, two) == ([0] * 12, [0] * 12)
        assert run(pipe, one) == ([1] * 12, [2] * 12)
        pipe.set_keep(None)
        assert run(pipe, two) == ([0, 1] * 6, [0, 3] * 6)


# ------------------------------------------------------------------ 5. the word seam, vectors_needed == 0

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40], ids=["compact8-zero-copy", "aos40"])
def test_word_seam_and_vn0_by_hand(gpu_scanner_factory, layout):
    p, frames, cases = pz.seam_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
        for keep, hand in cases:
            pipe.set_keep(keep)
            assert run(pipe, frames) == ([int(h >= p.clusters_needed) for h in hand], list(hand))
    p, frames, keep, hand = pz.vn0_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
        pipe.set_keep(keep)
        assert run(pipe, frames) == ([1], list(hand))          # a kept cell is active, an ignored one is not
        pipe.set_keep(None)
        assert run(pipe, frames) == ([1], [64])                # every cell of the grid active: x in [1, 8], 8 rows


# ------------------------------------------------------------------ 6. other grids

def test_4k_grid(gpu_scanner_factory):
    p, frames, keep, (want_f, want_c) = pz.uhd_case()
    s = gpu_scanner_factory(p)
    for layout in (m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40):
        with contextlib.closing(m.ScanPipe(s, 32400 * 3, 5, 2, layout=layout, centres=True)) as pipe:
            pipe.set_keep(keep)
            assert run(pipe, frames) == (want_f.tolist(), want_c.tolist())


def test_more_keep_words_than_lanes(gpu_scanner_factory):
    """4 x 1050 cells: the keep words of rows 1024.. are staged by the workgroup's second trip."""
    p, frames, keep, hand = pz.tall_case()
    s = gpu_scanner_factory(p)
    for layout in (m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40):
        with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
            pipe.set_keep(keep)
            assert run(pipe, frames) == ([1, 1], list(hand))
            pipe.set_keep(None)
            assert run(pipe, frames) == ([1, 1], [6, 2])


def test_grid_without_a_masked_form(gpu_scanner_factory):
    """960 x 540 cells: set_keep is MT_ERR_UNSUPPORTED with the grid named, and the pipe goes on scanning plainly."""
    p = m.ScanParams.from_config(3840, 2160, **pz.FINE_KW)
    s = gpu_scanner_factory(p)
    from mvtrim_amd import synth
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    b = m.FrameBatch.from_frames(frames)
    want = ob.scan_frames(ob.params_from_config(3840, 2160, **pz.FINE_KW), b.mv, b.frame_off, b.has_sd).tolist()
    assert want == [0, 1, 1]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(np.ones((p.grid_h, p.grid_w), dtype=bool))
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.has_keep is False
        feed_all(pipe, frames)
        assert [fl for _, fl, _ in pipe.drain()] == want


# ------------------------------------------------------------------ 7. mtgpu_scan_file --keep

MERGE_ENV = dict(MAX_GAP_SEC="0.5", PADDING_SEC="0.1", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="30",
                 VECTORS_NEEDED="1")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 90-frame recording as a .mtmv file, mask A as a .mtkeep file, a 320 x 240 recording."""
    from mvtrim_amd import synth
    d = tmp_path_factory.mktemp("pipe_zones")
    p, frames, pts, keep_a, _, want = pz.hd_case()
    spec = synth.spec_1080p(seed=17, sub=1)
    path = str(d / "hd.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, spec.tb_den, spec.fps, 90 / spec.fps, [spec.pts_ticks(i) for i in range(90)], list(frames))
    mask = str(d / "a.mtkeep")
    zones.save_keep(mask, keep_a)
    small = synth.StreamSpec(width=320, height=240, block=16, sub=1, fps=30.0, gop=15, seed=2)
    small.events = [synth.Event(2, 28, 5, 5, 3, 3, 8, 1)]
    other = str(d / "sd.mtmv")
    m.mvfile.write_mtmv(other, 320, 240, 1, small.tb_den, small.fps, 1.0, [small.pts_ticks(i) for i in range(30)],
                        [synth.gen_frame(small, i) for i in range(30)])
    env = dict(os.environ, **MERGE_ENV)
    for k in ("CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, other, env


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=3.0, max_gap_sec=0.5, padding_sec=0.1, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def test_scan_file_keep(gpu_scanner_factory, recording):
    path, mask, other, env = recording
    p, frames, pts, keep_a, _, want = pz.hd_case()
    s = gpu_scanner_factory(p)
    exe = os.path.join(PKG, "mtgpu_scan_file")
    fl, _, _ = s.scan_zones(m.FrameBatch.from_frames(list(frames)), [0, 90], zones.pack_keep(keep_a))
    want_seg, want_res = python_segments(s, fl, pts)
    out = subprocess.run([exe, path, "--threads", "2", "--keep", mask], check=True, capture_output=True, text=True, env=env, timeout=120)
    r = json.loads(out.stdout)
    assert r["segments"] == want_seg and r["motion_frames"] == int(fl.sum()) == int(want["a"][0].sum())
    assert r["do_cut"] == want_res["do_cut"] and r["ignored_cells"] == int((~keep_a).sum()) and r["frames_scanned"] == 90
    plain = json.loads(subprocess.run([exe, path, "--threads", "2"], check=True, capture_output=True, text=True, env=env,
                                      timeout=120).stdout)
    plain_seg, _ = python_segments(s, want["none"][0], pts)
    assert "ignored_cells" not in plain and plain["segments"] == plain_seg and plain["motion_frames"] == int(want["none"][0].sum())
    assert plain["segments"] != r["segments"] and plain["motion_frames"] > r["motion_frames"]
    # two inputs, the second with another grid: it fails with the parser's message, the first is unaffected
    out = subprocess.run([exe, path, other, "--threads", "2", "--streams", "1", "--keep", mask], capture_output=True, text=True,
                         env=env, timeout=120)
    assert out.returncode == 1, out.stdout + out.stderr
    jobs = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(jobs) == 1 and jobs[0]["input"] == path and jobs[0]["segments"] == want_seg and jobs[0]["motion_frames"] == r["motion_frames"]
    assert other in out.stderr and "line 2: the mask is for a 120x68 grid, this one is 20x15" in out.stderr
    # without --keep the second input scans
    out = subprocess.run([exe, path, other, "--threads", "2", "--streams", "1"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0 and len([ln for ln in out.stdout.splitlines() if ln.startswith("{")]) == 2, out.stdout + out.stderr


# ------------------------------------------------------------------ 8. one worker pool, several videos

def test_next_video_does_not_inherit_the_mask(gpu_scanner_factory, recording, tmp_path):
    """run_scan_pipeline three times on one pool of GpuBackends (tests/cpp/pipe_zones_two_videos.cpp): masked, plain,
    masked.  The second video's result is the unmasked one and its pipes carry no mask."""
    path, mask, _, env = recording
    p, frames, pts, keep_a, _, want = pz.hd_case()
    exe = str(tmp_path / "pipe_zones_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_zones_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, mask, "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 3
    for i, r in enumerate(runs):
        kv = dict(zip(r[0::2], r[1::2]))
        masked = i != 1
        w = want["a" if masked else "none"][0]
        ts = [float(t) for t in kv.get("timestamps", "").split(",") if t]
        assert ts == [pts[f] for f in range(90) if w[f]], i
        assert int(kv["motion_frames"]) == int(w.sum()) and int(kv["frames_scanned"]) == 90
        assert set(kv["has_keep"].split(",")) == {"1" if masked else "0"} and len(kv["has_keep"].split(",")) == 2
        assert (int(kv["keep"]) > 0) == masked


# ------------------------------------------------------------------ 9. launch scratch and profiling

def test_masked_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    """A masked submit keeps its work list in the batch's own block: a context that has run nothing but masked pipe
    batches has never reserved launch scratch.  With profiling on, every masked submit records one event triple."""
    p, one, two, keep = pz.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 4096, 4, 2, centres=True)) as pipe:
        pipe.set_keep(keep)
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, one) == ([1] * 12, [2] * 12)      # three batches of four frames
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


def test_plain_c_pipe_zones_example(tmp_path):
    exe = str(tmp_path / "pipe_zones_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_zones_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "with the zone:    motion frames 29, segments 1" in out.stdout and "without the zone: motion frames 58, segments 2" in out.stdout
