"""GPU tier (`-m gpu`): global-motion compensation carried through the pipe under its keep mask
(include/mtgpu_pipe_gmc.h; csrc/gmc_kernels.hip, the pipe form), the C++ host layer and mtgpu_scan_file.  Expected
values: numbers derived by hand and the model (tests/pipe_gmc_inputs.py; both checked without a GPU by
tests/test_pipe_gmc_host.py), and mtgpu_scan_frames_gmc / the plain and the masked pipe on the same frames for P1 - P4.
Every comparison is exact."""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import pipe_gmc_inputs as pg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES
LAYOUTS = [rec | zc | CE for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC)]
LAYOUT_IDS = ["-".join([r] + z) for r in ("compact8", "aos40") for z in ([], ["zero-copy"])]
VEC = _abi.MT_PIPE_REPORT_VECTOR


def feed_all(pipe, frames, pts=None):
    for i, f in enumerate(frames):
        pipe.feed(f, float(i) if pts is None else pts[i], tag=i)


def run(pipe, frames, pts=None):
    """Feed, drain -> (flags, counts) lists in tag order (the pipe returns submission order: asserted equal); counts is
    None in a pipe without MT_LAYOUT_CENTRES."""
    feed_all(pipe, frames, pts)
    if pipe._centres:
        out = pipe.drain_centres()
        assert [t for _, _, t, _ in out] == list(range(len(frames)))
        return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]
    out = pipe.drain()
    assert [t for _, _, t in out] == list(range(len(frames)))
    return [fl for _, fl, _ in out], None


def resident(s, frames, ms, q8):
    """mtgpu_scan_frames_gmc on the same frames -> (flags, centres, packed vectors) lists."""
    fl, ce, info = s.scan_gmc(m.FrameBatch.from_frames(list(frames)), ms, q8)
    return fl.tolist(), ce.tolist(), [pg.pack_vector(x, y) for x, y in zip(info["gx"].tolist(), info["gy"].tolist())]


# ------------------------------------------------------------------ 1. the rule bites

def test_the_rule_bites(gpu_scanner_factory):
    """The hand frames of pipe_gmc_inputs.hand_frames(), each against its hand-derived flag, centres and vector and
    against the model.  Case d separates "the mask reaches the estimate" from "the mask reaches only the active plane":
    without the keep bit in the estimate the mode stays 0 and the frame keeps its 40 centres."""
    p = pg.params()
    s = gpu_scanner_factory(p)
    h = pg.hand_frames()
    with contextlib.closing(m.ScanPipe(s, 8192, 2, 2, centres=True)) as pipe:
        assert pipe.gmc() is None
        for name, fr, kp, mode, (flag, centres, vec) in pg.HAND:
            keep = pg.KEEPS[kp]
            pipe.set_keep(keep)
            if mode == "plain":
                pipe.clear_gmc()
                assert run(pipe, [h[fr]]) == ([flag], [centres]) == pg.masked_plain(p, [h[fr]], keep), name
                continue
            mf, mc, mv = pg.model(p, [h[fr]], pg.MS, pg.Q8, keep)
            assert (mf, mc, mv) == ([flag], [centres], [pg.pack_vector(*vec)]), name
            pipe.set_gmc(pg.MS, pg.Q8, "centres")
            assert pipe.gmc() == (pg.MS, pg.Q8, "centres")
            assert run(pipe, [h[fr]]) == ([flag], [centres]), name
            pipe.set_gmc(pg.MS, pg.Q8, "vector")
            assert pipe.gmc() == (pg.MS, pg.Q8, "vector")
            got_f, got_v = run(pipe, [h[fr]])
            assert (got_f, [pipe.unpack_gmc_vector(got_v[0])]) == ([flag], [vec]), name


# ------------------------------------------------------------------ 2. P1 - P4 in every layout and batch shape

@pytest.fixture(scope="module")
def shapes_expected():
    """The model's answers for shapes_case(), once: {(ms, q8, masked): (flags, centres, vectors)}."""
    p, frames, keep = pg.shapes_case()
    return {(ms, q8, k): pg.model(p, frames, ms, q8, keep if k else None) for ms, q8 in pg.SETTINGS for k in (False, True)}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_p1_to_p4_in_every_layout_and_batch_shape(gpu_scanner_factory, shapes_expected, layout):
    p, frames, keep = pg.shapes_case()
    s = gpu_scanner_factory(p)
    n = len(frames)
    ones = np.ones((pg.GH, pg.GW), dtype=bool)
    geoms = [(40000, 1, 2), (70000, 4, 2), (200000, n, 2), (4096, 5, 3)]       # one frame; 4; exactly the capacity; growing batches
    for gi, (max_rec, max_fr, nbuf) in enumerate(geoms):
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout)) as pipe:
            plain = run(pipe, frames)
            pipe.set_keep(keep)
            masked = run(pipe, frames)
            pipe.set_keep(None)
            assert plain == pg.masked_plain(p, frames) and masked == pg.masked_plain(p, frames, keep)
            for ms, q8 in (pg.SETTINGS if gi == 1 else pg.SETTINGS[:2]):
                want = shapes_expected[(ms, q8, False)]
                res = resident(s, frames, ms, q8)
                assert res == want, (ms, q8)
                # P1: no keep plane == mtgpu_scan_frames_gmc; the vector report == the packed info of the resident call
                pipe.set_gmc(ms, q8, "centres")
                assert run(pipe, frames) == (res[0], res[1]), (max_fr, ms, q8)
                pipe.set_gmc(ms, q8, "vector")
                assert run(pipe, frames) == (res[0], res[2]), (max_fr, ms, q8)
                # P2: all ones == no keep plane
                pipe.set_keep(ones)
                assert run(pipe, frames) == (res[0], res[2]), (max_fr, ms, q8)
                # the model under the mask, both reports
                wantk = shapes_expected[(ms, q8, True)]
                pipe.set_keep(keep)
                assert run(pipe, frames) == (wantk[0], wantk[2]), (max_fr, ms, q8)
                pipe.set_gmc(ms, q8, "centres")
                got = run(pipe, frames)
                assert got == (wantk[0], wantk[1]), (max_fr, ms, q8)
                if ms == 0:                                   # P3: max_shift 0 == the pipe without compensation
                    assert got == masked and (res[0], res[1]) == plain
                elif gi == 1:
                    # P4: (gx, gy) of the resident call on the frames without their keep-0 records; the masked pipe fed the
                    # src-shifted frames gives the same centres
                    stripped = [None if f is None else pg.remove_masked(p, f, keep) for f in frames]
                    vec = resident(s, stripped, ms, q8)[2]
                    assert vec == wantk[2]
                    moved = [None if f is None else pg.shifted(f, *pg.unpack_vector(v)) for f, v in zip(frames, vec)]
                    assert all((a is None) == (b is None) for a, b in zip(frames, moved))     # every shift stays inside int16
                    pipe.clear_gmc()
                    assert run(pipe, moved) == got, (ms, q8)
                pipe.set_keep(None)
                pipe.clear_gmc()
            assert run(pipe, frames) == plain                  # enable == 0: the plain pipe again
    with contextlib.closing(m.ScanPipe(s, 40000, 1, 1, layout=layout)) as pipe:      # one frame through a pipe of one batch
        pipe.set_keep(keep)
        pipe.set_gmc(16, 64, "vector")
        wantk = shapes_expected[(16, 64, True)]
        for i in (1, 4, 0, 5):
            assert run(pipe, frames[i:i + 1]) == (wantk[0][i:i + 1], wantk[2][i:i + 1]), i


# ------------------------------------------------------------------ 3. stale results in the pinned block

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", ["centres", "vector"])
def test_no_stale_results_in_a_reused_pinned_block(gpu_scanner_factory, layout, report):
    """n_buffers = 1, zero-copy: batch 1 leaves flag 1 / 30 centres / (9, 3) in every slot of the pinned block; batch 2
    goes into the same slots and every flag and count must read the new value — from the kernel's one exit, with and
    without a centre, and from the planning kernel."""
    p, one, two, h1, h2 = pg.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 16384, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_gmc(pg.MS, pg.Q8, report)
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, two) == (h2["flags"], h2[report])
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, list(reversed(two))) == (list(reversed(h2["flags"])), list(reversed(h2[report])))


# ------------------------------------------------------------------ 4. limits

def _limit_run(s, p, gw, gh, keep):
    import derived_cliff_inputs as dc
    sh = dc.shift_of(gw, gh)
    clear = [(1, gh // 2), (2, gh // 2)]
    frames = pg.limit_frames(gw, gh, sh, clear)
    nrec = max(len(f) for f in frames if f is not None)
    out = {}
    with contextlib.closing(m.ScanPipe(s, 2 * nrec, 2, 2, centres=True)) as pipe:
        if keep is not None:
            pipe.set_keep(keep)
        pipe.set_gmc(16, 128, "centres")
        out["centres"] = run(pipe, frames)
        pipe.set_gmc(16, 128, "vector")
        out["vector"] = run(pipe, frames)
    return frames, out


def test_limit_shape_only_the_compensated_scan_accepts(gpu_scanner_factory):
    """(i) wide-65 x 584, a limit shape of the compensated scan that mtgpu_zones_preview rejects: set_gmc is OK, set_keep
    is MT_ERR_UNSUPPORTED, and the pipe runs unmasked compensation equal to the model.  By hand: the pan (7, -3) is
    cancelled (0 centres); the object pair keeps (5, 0): 2 centres; the still pair keeps (-7, 3): 2 centres."""
    import derived_cliff_inputs as dc
    gw, gh, _ = next(v for k, v in dc.shapes("gmc").items() if k.startswith("tall-65x"))
    p = dc.grid_params(gw, gh, vectors_needed=1, mv_threshold_sq=16.0, clusters_needed=2)
    assert dc.kernel_preview("gmc", p) is not None and dc.kernel_preview("zones", p) is None
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2)) as pipe:
        pipe.set_gmc()
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(np.ones((gh, gw), dtype=bool))
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and f"{gw}x{gh}" in str(e.value)
        assert not pipe.has_keep and pipe.gmc() == (16, 128, "centres")
    frames, out = _limit_run(s, p, gw, gh, None)
    want = pg.model(p, frames, 16, 128)
    assert (want[0], want[1]) == ([0, 1, 1, 0], [0, 2, 2, 0])
    assert want[2] == [pg.pack_vector(7, -3)] * 3 + [0]
    assert out["centres"] == (want[0], want[1]) and out["vector"] == (want[0], want[2])


def test_limit_shape_of_the_masked_scan(gpu_scanner_factory):
    """(ii) tall-65 x 530, a limit shape of the masked scan: masked compensation runs there and equals the model.  By
    hand, with the still pair's cells cleared: 0, 2, 0 centres."""
    import derived_cliff_inputs as dc
    gw, gh, _ = next(v for k, v in dc.shapes("zones").items() if k.startswith("tall-65x"))
    p = dc.grid_params(gw, gh, vectors_needed=1, mv_threshold_sq=16.0, clusters_needed=2)
    assert dc.kernel_preview("gmc", p) is not None and dc.kernel_preview("zones", p) is not None
    s = gpu_scanner_factory(p)
    keep = np.ones((gh, gw), dtype=bool)
    keep[gh // 2, 1] = keep[gh // 2, 2] = False
    frames, out = _limit_run(s, p, gw, gh, keep)
    want = pg.model(p, frames, 16, 128, keep)
    assert (want[0], want[1]) == ([0, 1, 0, 0], [0, 2, 0, 0])
    assert out["centres"] == (want[0], want[1]) and out["vector"] == (want[0], want[2])


def test_row_banded_grid_is_unsupported(gpu_scanner_factory):
    """(iii) 960 x 540 cells: set_gmc is MT_ERR_UNSUPPORTED with the grid named, the setting stays off and the pipe goes
    on scanning plainly."""
    from mvtrim_amd import synth
    p = m.ScanParams.from_config(3840, 2160, **pg.FINE_KW)
    s = gpu_scanner_factory(p)
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        before = run(pipe, frames)[0]
        assert before == s.check_frames(m.FrameBatch.from_frames(frames)).tolist() == [0, 1, 1]
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc()
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.gmc() is None and m.load_library().mtgpu_pipe_gmc(pipe._pipe, None, None, None) == 0
        assert run(pipe, frames)[0] == before


# ------------------------------------------------------------------ 5. contracts

def test_bad_arguments_change_nothing(gpu_scanner_factory):
    p = pg.params()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    h = pg.hand_frames()
    frames = [h["a"], h["d"]]
    with contextlib.closing(m.ScanPipe(s, 8192, 2, 2)) as pipe:                # no MT_LAYOUT_CENTRES
        bad = [((1, -1, 128, 0), "max_shift"), ((1, 128, 128, 0), "max_shift"), ((1, 16, -1, 0), "min_share_q8"),
               ((1, 16, 257, 0), "min_share_q8"), ((1, 16, 128, _abi.MT_PIPE_REPORT_LARGEST), "report"), ((1, 16, 128, 3), "report"),
               ((1, 16, 128, -1), "report"), ((1, 16, 128, VEC), "MT_LAYOUT_CENTRES")]
        for state in (None, (4, 200, "centres")):
            if state:
                pipe.set_gmc(*state)
            for args, word in bad:
                assert lib.mtgpu_pipe_set_gmc(pipe._pipe, *args) == _abi.MT_ERR_INVALID, args
                assert word in lib.mtgpu_last_error().decode(), args
                assert pipe.gmc() == state
        assert lib.mtgpu_pipe_set_gmc(None, 1, 16, 128, 0) == _abi.MT_ERR_INVALID and lib.mtgpu_pipe_gmc(None, None, None, None) == -1
        with pytest.raises(ValueError):
            pipe.set_gmc(16, 128, "largest")
        pipe.set_gmc()
        assert run(pipe, frames)[0] == [0, 1]
        assert lib.mtgpu_pipe_set_gmc(pipe._pipe, 0, 999, -5, 77) == _abi.MT_OK and pipe.gmc() is None     # ignored at enable 0
        a, b, c = ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_int(7)
        assert lib.mtgpu_pipe_gmc(pipe._pipe, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
        assert (a.value, b.value, c.value) == (7, 7, 7)
        assert run(pipe, frames)[0] == [1, 1]
    with contextlib.closing(m.ScanPipe(s, 8192, 2, 2, centres=True)) as pipe:
        pipe.set_gmc(5, 100, "vector")
        assert lib.mtgpu_pipe_gmc(pipe._pipe, None, None, None) == 1 and pipe.gmc() == (5, 100, "vector")
        pipe.clear_gmc()
        pipe.set_gmc()                                                         # the report was reset at enable 0
        assert pipe.gmc() == (16, 128, "centres")


def test_busy_and_one_pipe_two_recordings(gpu_scanner_factory):
    p, frames, keep = pg.shapes_case()
    frames = [f for f in frames if f is None or len(f) < 10000]                 # the hand frames and the empty ones
    n = len(frames)
    s = gpu_scanner_factory(p)
    plain = pg.masked_plain(p, frames)
    a = pg.model(p, frames, 16, 128)
    b = pg.model(p, frames, 16, 128, keep)
    assert plain[0] != a[0] != b[0]
    with contextlib.closing(m.ScanPipe(s, 16384, 4, 3, centres=True)) as pipe:
        pipe.set_gmc(16, 128, "centres")
        assert run(pipe, frames) == (a[0], a[1])
        feed_all(pipe, frames[:3])                                              # a batch being filled
        for call in (lambda: pipe.set_gmc(3, 0, "vector"), pipe.clear_gmc):
            with pytest.raises(m.MtgpuError) as e:
                call()
            assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value) and pipe.gmc() == (16, 128, "centres")
        for i in range(3, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (a[0], a[1])
        feed_all(pipe, frames[:6])                                              # 4 submitted, 2 being filled
        pipe._submit()
        assert pipe._cur is None and pipe._inflight >= 1
        with pytest.raises(m.MtgpuError) as e:
            pipe.clear_gmc()
        assert e.value.code == _abi.MT_ERR_BUSY and "in flight" in str(e.value) and pipe.gmc() == (16, 128, "centres")
        for i in range(6, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (a[0], a[1])
        # the next recording: another setting and a mask
        pipe.set_keep(keep)
        pipe.set_gmc(16, 128, "vector")
        assert run(pipe, frames) == (b[0], b[2])
        pipe.clear_gmc()
        assert run(pipe, frames) == pg.masked_plain(p, frames, keep)            # enable == 0: the masked pipe, bit for bit
        pipe.set_keep(None)
        assert run(pipe, frames) == plain


def test_keep_and_gmc_commute_and_blobs_are_refused(gpu_scanner_factory):
    p = pg.params()
    s = gpu_scanner_factory(p)
    h = pg.hand_frames()
    frames = [h["c"], h["d"], None, h["e"]]
    keep = pg.shapes_case()[2]
    want = pg.model(p, frames, 16, 128, keep)
    results = []
    for order in ("keep-first", "gmc-first"):
        with contextlib.closing(m.ScanPipe(s, 8192, 2, 2, centres=True)) as pipe:
            if order == "keep-first":
                pipe.set_keep(keep)
                pipe.set_gmc(16, 128, "vector")
            else:
                pipe.set_gmc(16, 128, "vector")
                pipe.set_keep(keep)
            assert pipe.has_keep and pipe.gmc() == (16, 128, "vector")
            x = run(pipe, frames)
            pipe.set_keep(None)
            assert pipe.gmc() == (16, 128, "vector")
            y = run(pipe, frames)
            results.append((x, y))
    assert results[0] == results[1]
    assert results[0][0] == (want[0], want[2])
    nomask = pg.model(p, frames, 16, 128)
    assert results[0][1] == (nomask[0], nomask[2])
    with contextlib.closing(m.ScanPipe(s, 8192, 2, 2, centres=True)) as pipe:
        pipe.set_blobs(3, "largest")
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc()
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value)
        assert pipe.gmc() is None and pipe.blobs == (3, "largest")
        blob_run = run(pipe, frames)
        pipe.set_blobs(0)
        pipe.set_gmc(16, 128, "centres")
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_blobs(3, "largest")
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value)
        assert pipe.blobs is None and pipe.gmc() == (16, 128, "centres")
        pipe.set_blobs(0)                                                       # off is always accepted
        assert run(pipe, frames) == (nomask[0], nomask[1])
        pipe.clear_gmc()
        pipe.set_blobs(3, "largest")
        assert run(pipe, frames) == blob_run


def test_gmc_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    p, one, two, h1, h2 = pg.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 16384, 1, 2, centres=True)) as pipe:
        pipe.set_keep(pg.ONES)
        pipe.set_gmc(pg.MS, pg.Q8, "vector")
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, one) == (h1["flags"], h1["vector"])           # three batches of one frame
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


# ------------------------------------------------------------------ 6. mtgpu_scan_file, the host layer, the example

MERGE_ENV = dict(MAX_GAP_SEC="0.1", PADDING_SEC="0.04", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="25")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 40-frame shaking recording with its overlay as a .mtmv file, the overlay's mask as a .mtkeep file."""
    d = tmp_path_factory.mktemp("pipe_gmc")
    p, frames, pts, keep = pg.recording_case()
    path = str(d / "shake.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, pg.REC_FPS, pg.REC_FRAMES / pg.REC_FPS, list(range(pg.REC_FRAMES)), list(frames))
    mask = str(d / "overlay.mtkeep")
    zones.save_keep(mask, keep)
    env = dict(os.environ, **MERGE_ENV)
    for k in ("CLUSTERS_NEEDED", "VECTORS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, env


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=pg.REC_FRAMES / pg.REC_FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def scan_file(env, path, *args):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2"] + list(args), capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def top_vectors(vectors):
    """[[gx, gy, frames]] of the non-zero packed vectors, most frequent first, then by (gx, gy); at most 8."""
    seen = {}
    for v in vectors:
        if v:
            seen[pg.unpack_vector(v)] = seen.get(pg.unpack_vector(v), 0) + 1
    return [[gx, gy, n] for (gx, gy), n in sorted(seen.items(), key=lambda kv: (-kv[1], kv[0]))][:8]


def test_scan_file_gmc_keep_and_vectors(gpu_scanner_factory, recording):
    path, mask, env = recording
    p, frames, pts, keep = pg.recording_case()
    s = gpu_scanner_factory(p)
    plain = scan_file(env, path)
    assert plain["motion_frames"] == sum(pg.masked_plain(p, frames)[0]) and "gmc" not in plain
    seen = {}
    for keep_args, kp in (([], None), (["--keep", mask], keep)):
        fl, ce, ve = pg.model(p, frames, 16, 128, kp)
        want_seg, want_res = python_segments(s, fl, pts)
        r = scan_file(env, path, "--gmc", *keep_args)
        assert r["motion_frames"] == sum(fl) and r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"], keep_args
        assert r["frames_scanned"] == pg.REC_FRAMES and ("ignored_cells" in r) == bool(keep_args) and "gmc" not in r
        seen[bool(keep_args)] = r
        c = scan_file(env, path, "--gmc", "--centres", *keep_args)
        assert [n for _, n in c["centres"]] == ce and c["segments"] == want_seg
        v = scan_file(env, path, "--gmc-vectors", *keep_args)
        assert v["segments"] == want_seg and "centres" not in v
        moved = sum(1 for x in ve if x)
        assert v["gmc"] == {"frames": pg.REC_FRAMES, "compensated_frames": moved, "compensated_share": moved / pg.REC_FRAMES,
                            "vectors": top_vectors(ve)}
    assert seen[False]["motion_frames"] == plain["motion_frames"]            # the overlay keeps every moving frame flagged
    assert seen[True]["motion_frames"] == 10 and seen[True]["segments"] != plain["segments"]
    # the two parameters each imply --gmc
    fl = pg.model(p, frames, 2, 128, keep)[0]
    r = scan_file(env, path, "--gmc-max-shift", "2", "--keep", mask)
    assert r["motion_frames"] == sum(fl) != 10 and r["segments"] == python_segments(s, fl, pts)[0]
    fl = pg.model(p, frames, 16, 256, None)[0]
    r = scan_file(env, path, "--gmc-min-share-q8", "256")
    assert r["motion_frames"] == sum(fl) and r["segments"] == python_segments(s, fl, pts)[0]
    # usage errors: nothing is decoded
    exe = os.path.join(PKG, "mtgpu_scan_file")
    for args, text in ((["--gmc", "--min-blob-cells", "3"], "--gmc cannot be combined with --min-blob-cells or --sweep-blobs"),
                       (["--sweep-blobs", "4", "--gmc-max-shift", "5"], "--gmc cannot be combined with --min-blob-cells or --sweep-blobs"),
                       (["--gmc-vectors", "--centres"], "--gmc-vectors cannot be combined with --centres or --sweep"),
                       (["--gmc-vectors", "--sweep", "2,3"], "--gmc-vectors cannot be combined with --centres or --sweep")):
        out = subprocess.run([exe, path, "--threads", "2"] + args, capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 2 and text in out.stderr and out.stdout == "", (args, out.stderr)


def test_next_video_does_not_inherit_the_gmc_setting(recording, tmp_path):
    """run_scan_pipeline on one pool of GpuBackends (tests/cpp/pipe_gmc_two_videos.cpp): compensated, plain, compensated
    at max_shift 3 with the vectors reported, and compensation together with blobs, refused before any decode."""
    path, _, env = recording
    p, frames, pts, _ = pg.recording_case()
    exe = str(tmp_path / "pipe_gmc_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_gmc_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 4
    want = [pg.model(p, frames, 16, 128), pg.masked_plain(p, frames) + ([0] * len(frames),), pg.model(p, frames, 3, 128)]
    for i, r in enumerate(runs[:3]):
        kv = dict(zip(r[0::2], r[1::2]))
        fl, _, ve = want[i]
        ts = [float(t) for t in kv["timestamps"].split(",") if t != "-"]
        assert ts == [pts[f] for f in range(pg.REC_FRAMES) if fl[f]], i
        assert int(kv["motion_frames"]) == sum(fl) and int(kv["frames_scanned"]) == pg.REC_FRAMES
        assert kv["gmc"].split(",") == [("16", "-1", "3V")[i]] * 2
        if i == 2:
            assert int(kv["moved"]) == sum(1 for x in ve if x)
            assert kv["top"] == ",".join("%d:%d:%d" % tuple(t) for t in top_vectors(ve))
        else:
            assert kv["moved"] == "0" and kv["top"] == "-"
    assert want[0][0] != want[2][0] or want[0][2] != want[2][2]
    assert runs[3][:6] == ["run", "3", "rc", "1", "frames_scanned", "0"] and "not together yet" in " ".join(runs[3])


def test_plain_c_pipe_gmc_example(tmp_path):
    exe = str(tmp_path / "pipe_gmc_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_gmc_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plain scan:                       motion frames 290" in out.stdout
    assert "compensated, no mask:             motion frames 290" in out.stdout
    assert "compensated, the clock ignored:   motion frames 29" in out.stdout
