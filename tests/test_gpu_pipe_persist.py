"""GPU tier (`-m gpu`): the largest blob's box through the pipe (include/mtgpu_pipe_boxes.h; the boxed pipe forms of
csrc/blobs_kernels.hip and csrc/gmc_blobs_kernels.hip) and persistence on the decode path (the C++ host layer and
mtgpu_scan_file).  Expected values: the flood-fill model and the resident calls for boxes (tests/blobs_model.py,
scan_blobs / scan_gmc_blobs), tests/persist_model.py for the rule, merge_segments(job_semantics=True) for segments
(tests/pipe_persist_inputs.py; checked without a GPU by tests/test_pipe_persist_host.py).  Every comparison is exact."""
import contextlib
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import persist_inputs as pi
import persist_model as pmod
import pipe_gmc_inputs as pgi
import pipe_persist_inputs as pp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE, BX = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES, m.LAYOUT_BOXES
LAYOUTS = [rec | zc | ce for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC) for ce in (0, CE)]
LAYOUT_IDS = ["-".join([r] + z + c) for r in ("compact8", "aos40") for z in ([], ["zero-copy"]) for c in ([], ["centres"])]
NO_BOX = pp.NO_BOX


def run_boxes(pipe, frames):
    """Feed, drain_boxes -> (flags, counts or None, boxes) in tag order (asserted equal to submission order)."""
    for i, f in enumerate(frames):
        pipe.feed(f, float(i), tag=i)
    out = pipe.drain_boxes()
    assert [t for _, _, t, _, _ in out] == list(range(len(frames)))
    counts = [c for _, _, _, c, _ in out]
    return [fl for _, fl, _, _, _ in out], (counts if pipe._centres else None), [b for _, _, _, _, b in out]


def run_plain(pipe, frames):
    for i, f in enumerate(frames):
        pipe.feed(f, float(i), tag=i)
    if pipe._centres:
        out = pipe.drain_centres()
        return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]
    return [fl for _, fl, _ in pipe.drain()], None


def box_rows(a):
    return [tuple(int(v) for v in r) for r in np.stack([a[k] for k in ("x0", "y0", "x1", "y1")], axis=1).tolist()]


def where_flagged(boxes, flags):
    return [b if fl else NO_BOX for b, fl in zip(boxes, flags)]


# ------------------------------------------------------------------ 1. boxes equal the resident call's

@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_blob_pipe_boxes_equal_the_resident_call(gpu_scanner_factory, layout):
    """23 frames in batches of 5 under three settings, with and without the keep mask: wherever the flag is set the box
    is the model's and mtgpu_scan_frames_blobs'; everywhere else drain_boxes hands out the no-blob box; flags and counts
    are those of the unboxed pipe."""
    frames = pp.all_frames()
    keep = pp.keep_plane()
    for name, (p, mb) in pp.settings().items():
        s = gpu_scanner_factory(p)
        for masked in (False, True):
            want = pp.expected(name, masked)
            b = m.FrameBatch.from_frames(list(frames))
            r = s.scan_blobs(b, mb, [0, len(frames)], zones.pack_keep(keep)) if masked else s.scan_blobs(b, mb)
            assert r["flags"].tolist() == want["flags"] and box_rows(r["box"]) == want["model_box"], (name, masked)
            assert sum(want["flags"]) >= 5 and 0 in want["flags"]
            with contextlib.closing(m.ScanPipe(s, 512, pp.MAX_FRAMES, 2, layout=layout, boxes=True)) as pipe, \
                    contextlib.closing(m.ScanPipe(s, 512, pp.MAX_FRAMES, 2, layout=layout)) as bare:
                st = _abi.PipeStatsC()
                _abi.check(pipe._lib.mtgpu_pipe_get_stats(pipe._pipe, C.byref(st)))
                assert st.layout == layout | BX
                for q in (pipe, bare):
                    if masked:
                        q.set_keep(keep)
                    q.set_blobs(mb, "largest" if layout & CE else "centres")
                fl, cnt, boxes = run_boxes(pipe, frames)
                assert fl == want["flags"], (name, masked)
                assert boxes == want["box"] == where_flagged(box_rows(r["box"]), fl), (name, masked)
                assert cnt == (want["largest"] if layout & CE else None)
                assert (fl, cnt) == run_plain(bare, frames)
    # the hand values: the ties and the blob over every analysed row
    w = pp.expected("cn1", False)["box"]
    assert w[17] == (60, 40, 63, 40) and w[20] == (20, 10, 22, 11) and w[21] == (80, 10, 82, 11) and w[22] == (50, 0, 51, 67)
    assert pp.expected("margin3", False)["box"][22] == (50, 3, 51, 64)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_pair_pipe_boxes_equal_the_resident_call(gpu_scanner_factory, layout):
    """The compensated blob mode: with max_shift 0 on the same 23 frames (equal to the blob scan), and on the shaking
    synthetic stream of pipe_gmc_inputs.shapes_case against mtgpu_scan_frames_gmc_blobs, with and without the keep mask."""
    report = "largest" if layout & CE else "centres"
    frames = pp.all_frames()
    p, mb = pp.settings()["margin3"]
    s = gpu_scanner_factory(p)
    want = pp.expected("margin3", False)
    r = s.scan_gmc_blobs(m.FrameBatch.from_frames(list(frames)), 0, 128, mb)
    assert r["flags"].tolist() == want["flags"] and box_rows(r["box"]) == want["model_box"]
    with contextlib.closing(m.ScanPipe(s, 512, pp.MAX_FRAMES, 2, layout=layout, boxes=True)) as pipe, \
            contextlib.closing(m.ScanPipe(s, 512, pp.MAX_FRAMES, 2, layout=layout)) as bare:
        for q in (pipe, bare):
            q.set_gmc_blobs(mb, 0, 128, report)
        fl, cnt, boxes = run_boxes(pipe, frames)
        assert fl == want["flags"] and boxes == want["box"] and cnt == (want["largest"] if layout & CE else None)
        assert (fl, cnt) == run_plain(bare, frames)
    p, frames, keep = pgi.shapes_case()
    s = gpu_scanner_factory(p)
    big = 2 * max(len(f) for f in frames if f is not None)
    for masked in (False, True):
        args = ([0, len(frames)], zones.pack_keep(np.asarray(keep, dtype=bool))) if masked else ()
        r = s.scan_gmc_blobs(m.FrameBatch.from_frames(list(frames)), 16, 128, 2, *args)
        fl0 = r["flags"].tolist()
        assert fl0[1] and fl0[6] and fl0[11] and 0 in fl0          # the three shaking frames are flagged
        with contextlib.closing(m.ScanPipe(s, big, pp.MAX_FRAMES, 2, layout=layout, boxes=True)) as pipe, \
                contextlib.closing(m.ScanPipe(s, big, pp.MAX_FRAMES, 2, layout=layout)) as bare:
            for q in (pipe, bare):
                if masked:
                    q.set_keep(keep)
                q.set_gmc_blobs(2, 16, 128, report)
            fl, cnt, boxes = run_boxes(pipe, frames)
            assert fl == fl0 and boxes == where_flagged(box_rows(r["box"]), fl0), masked
            assert cnt == (r["largest"].tolist() if layout & CE else None)
            assert (fl, cnt) == run_plain(bare, frames)


# ------------------------------------------------------------------ 2. no stale box in a reused block

@pytest.mark.parametrize("mode", ["blobs", "pair"])
@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC | CE], ids=["compact8-zero-copy", "aos40-zero-copy-centres"])
def test_no_stale_box_in_a_reused_pinned_block(gpu_scanner_factory, layout, mode):
    """n_buffers = 1, zero-copy: batch 2 goes into the slots of batch 1 with its blobs elsewhere and quiet frames where
    batch 1 had blobs.  Every flagged frame of batch 2 has batch 2's box (the quiet ones are unspecified in the block and
    read as the no-blob box through drain_boxes)."""
    p, mb, one, two, b1, f2, b2 = pp.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 256, 4, 1, layout=layout, boxes=True)) as pipe:
        if mode == "blobs":
            pipe.set_blobs(mb)
        else:
            pipe.set_gmc_blobs(mb, 0, 128)
        for _ in range(2):
            fl, _, boxes = run_boxes(pipe, one)
            assert fl == [1, 1, 1, 1] and boxes == b1
            fl, _, boxes = run_boxes(pipe, two)
            assert fl == f2 and boxes == b2


# ------------------------------------------------------------------ 3. refusals change nothing

def test_refusals_change_nothing(gpu_scanner_factory):
    p, mb, one, two, b1, f2, b2 = pp.stale_case()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID

    def boxes_of(h):
        bp = C.c_void_p(1)
        rc = lib.mtgpu_batch_boxes(h, C.byref(bp))
        return rc, bp.value, lib.mtgpu_last_error().decode()

    def submit_collect(pipe, frames):
        for i, f in enumerate(frames):
            pipe.feed(f, float(i), tag=i)
        pipe._submit()
        h, fl, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _abi.check(lib.mtgpu_pipe_collect(pipe._pipe, C.byref(h), C.byref(fl), None, None, C.byref(n)))
        flags = np.ctypeslib.as_array(C.cast(fl, C.POINTER(C.c_uint8)), (n.value,)).tolist()
        return h, flags

    def release(pipe, h):
        _abi.check(lib.mtgpu_pipe_release(pipe._pipe, h))
        pipe._inflight -= 1

    # an unboxed pipe
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2, centres=True)) as pipe:
        pipe.set_blobs(mb)
        h, flags = submit_collect(pipe, two)
        rc, ptr, msg = boxes_of(h)
        release(pipe, h)
        assert (rc, ptr) == (inv, None) and "MT_LAYOUT_BOXES" in msg and flags == f2
        with pytest.raises(m.MtgpuError) as e:
            pipe.drain_boxes()
        assert e.value.code == inv and "LAYOUT_BOXES" in str(e.value)
        assert run_plain(pipe, two)[0] == f2
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2, boxes=True)) as pipe:
        # before collect: being filled, in flight
        h = C.c_void_p()
        _abi.check(lib.mtgpu_pipe_acquire(pipe._pipe, C.byref(h)))
        rc, ptr, msg = boxes_of(h)
        assert (rc, ptr) == (inv, None) and "collected" in msg
        _abi.check(lib.mtgpu_pipe_release(pipe._pipe, h))
        # the plain, the masked and the compensated mode of a boxed pipe: the same flags as ever, no boxes
        plain = s.check_frames(m.FrameBatch.from_frames(list(two))).tolist()
        for setup, undo in ((lambda: None, lambda: None), (lambda: pipe.set_keep(np.ones((pp.GH, pp.GW), dtype=bool)), lambda: pipe.set_keep(None)),
                            (lambda: pipe.set_gmc(0, 128), pipe.clear_gmc)):
            setup()
            h, flags = submit_collect(pipe, two)
            rc, ptr, msg = boxes_of(h)
            release(pipe, h)
            assert (rc, ptr) == (inv, None) and "mtgpu_pipe_set_blobs" in msg and "mtgpu_pipe_set_gmc_blobs" in msg
            assert flags == plain
            for i, f in enumerate(two):
                pipe.feed(f, float(i), tag=i)
            with pytest.raises(m.MtgpuError) as e:
                pipe.drain_boxes()
            assert e.value.code == inv and "mtgpu_pipe_set_blobs" in str(e.value)
            undo()
        # and the pipe goes on: a blob submit gives boxes, and after release the handle is refused again
        pipe.set_blobs(mb)
        h, flags = submit_collect(pipe, two)
        bp = C.c_void_p()
        assert lib.mtgpu_batch_boxes(h, C.byref(bp)) == _abi.MT_OK and bp.value and bp.value % 8 == 0
        got = np.ctypeslib.as_array(C.cast(bp, C.POINTER(C.c_uint16)), (4, 4)).tolist()
        assert flags == f2 and [tuple(got[i]) for i in (0, 3)] == [b2[0], b2[3]]
        release(pipe, h)
        rc, ptr, msg = boxes_of(h)
        assert (rc, ptr) == (inv, None) and "collected" in msg
        assert run_boxes(pipe, one) == ([1, 1, 1, 1], None, b1)
    # layout 16 and above
    out = C.c_void_p()
    for layout in (16, 16 | BX, 31, -1):
        assert lib.mtgpu_pipe_create_layout(s._ctx, 256, 4, 2, layout, C.byref(out)) == inv and not out.value
        assert "MT_LAYOUT_BOXES" in lib.mtgpu_last_error().decode()
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2, layout=m.LAYOUT_AOS40 | ZC | CE | BX)) as pipe:
        pipe.set_blobs(mb, "largest")
        assert run_boxes(pipe, two) == (f2, [12, 0, 0, 12], b2)


# ------------------------------------------------------------------ 4. one profile triple, no ring scratch

@pytest.mark.parametrize("mode", ["blobs", "pair"])
def test_boxed_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory, mode):
    p, mb, one, two, b1, f2, b2 = pp.stale_case()
    s = m.MotionScanner(p, device=0)                    # a context of its own: nothing else has launched on it
    try:
        high0 = s.stats()["pool_reserved_high"]
        with contextlib.closing(m.ScanPipe(s, 256, 1, 2, centres=True, boxes=True)) as pipe:
            if mode == "blobs":
                pipe.set_blobs(mb, "largest")
            else:
                pipe.set_gmc_blobs(mb, 0, 128, "largest")
            s.profile(True)
            try:
                s.profile_read()
                assert run_boxes(pipe, one) == ([1, 1, 1, 1], [12, 12, 12, 8], b1)      # four batches of one frame
                r = s.profile_read()
            finally:
                s.profile(False)
            assert r["launches"] == 4 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
            assert s.stats()["pool_reserved_high"] == high0
    finally:
        s.close()


# ------------------------------------------------------------------ mtgpu_scan_file

CONFIG_VARS = ("CLUSTERS_NEEDED", "VECTORS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING",
               "MAX_GAP_SEC", "PADDING_SEC", "MIN_SAVINGS_PCT", "CHUNK_DURATION_SEC", "TARGET_FPS")


def tool_env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in CONFIG_VARS}
    env.update({k: str(v) for k, v in kw.items()})
    return env


def scan_file(env, path, *args, threads=2):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", str(threads), "--timestamps"] + [str(a) for a in args],
                         capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def merged(s, ts, duration, max_gap, padding):
    mp = m.MergeParams(duration=duration, max_gap_sec=max_gap, padding_sec=padding, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(ts, dtype=np.float64), mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def what_counts(r):
    """What must not depend on chunking or on the number of workers."""
    return {k: r[k] for k in ("timestamps", "motion_frames", "n_timestamps", "segments", "do_cut", "saved_pct", "frames_scanned",
                              "frames_before_persist", "min_run", "max_dropout")}


# ------------------------------------------------------------------ 5. the seams

SEAM_MERGE = dict(MAX_GAP_SEC="0.15", PADDING_SEC="0.05", MIN_SAVINGS_PCT="5", VECTORS_NEEDED="1")


def write_seam_recording(path, extra_quiet=()):
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 10, pp.SEAM_FPS, pp.SEAM_FRAMES / pp.SEAM_FPS, list(range(pp.SEAM_FRAMES)),
                        list(pp.seam_frames(extra_quiet)))


def test_runs_cross_chunk_borders_and_key_frames(gpu_scanner_factory, tmp_path):
    """40 frames at 10 fps, key frames at 0, 20, 30, motion in 8 9 10 | 19 (20) 21 22 | 33.  With chunks of one second the
    borders fall at frames 10, 20 and 30: inside the first run, on the key frame inside the second.  --min-run 3 keeps
    exactly 8 9 10 19 21 22 whatever the chunking and the number of workers: a rule applied per chunk or per batch keeps
    neither run whole."""
    s = gpu_scanner_factory(m.ScanParams.from_config(1920, 1080, vectors_needed=1))
    path = str(tmp_path / "seams.mtmv")
    write_seam_recording(path)
    pts = pp.seam_pts()
    dur = pp.SEAM_FRAMES / pp.SEAM_FPS
    kept, runs = pp.seam_expected(3, 0)
    assert tuple(kept) == pp.SEAM_KEPT and [runs[f] for f in pp.SEAM_M] == [3, 3, 3, 3, 3, 3, 1]
    want_seg, want_res = merged(s, [pts[f] for f in kept], dur, 0.15, 0.05)
    assert len(want_seg) == 3                                          # 0.8 .. 1.0 | 1.9 | 2.1 .. 2.2
    plain = scan_file(tool_env(CHUNK_DURATION_SEC=1, **SEAM_MERGE), path)
    assert plain["timestamps"] == [pts[f] for f in pp.SEAM_M] and "min_run" not in plain and "frames_before_persist" not in plain
    for off in (["--min-run", 0], ["--min-run", 1]):
        again = scan_file(tool_env(CHUNK_DURATION_SEC=1, **SEAM_MERGE), path, *off)
        assert sorted(again) == sorted(plain) and all(again[k] == plain[k] for k in plain if not k.endswith("_us"))
    first = None
    for chunk in (0.5, 1, 1000):
        for threads in (1, 3):
            r = scan_file(tool_env(CHUNK_DURATION_SEC=chunk, **SEAM_MERGE), path, "--min-run", 3, threads=threads)
            assert r["timestamps"] == [pts[f] for f in kept], (chunk, threads)
            assert r["motion_frames"] == 6 and r["frames_before_persist"] == 7 and r["frames_scanned"] == 40
            assert r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"] and r["min_run"] == 3 and r["max_dropout"] == 0
            assert "reach" not in r and "runs" not in r and "sweep_min_run" not in r
            first = first or what_counts(r)
            assert what_counts(r) == first, (chunk, threads)
    # one quiet frame inside a run: frame 9 analysed and quiet.  MIN_RUN 2: without a dropout 8 and 10 are alone, with
    # --max-dropout 1 they are one run of two
    path2 = str(tmp_path / "dropout.mtmv")
    write_seam_recording(path2, extra_quiet=(9,))
    for drop, want in ((0, [19, 21, 22]), (1, [8, 10, 19, 21, 22])):
        assert pp.seam_expected(2, drop, (9,))[0] == want
        r = scan_file(tool_env(CHUNK_DURATION_SEC=1, **SEAM_MERGE), path2, "--min-run", 2, "--max-dropout", drop, threads=3)
        assert r["timestamps"] == [pts[f] for f in want] and r["max_dropout"] == drop and r["frames_before_persist"] == 6
        assert r["segments"] == merged(s, [pts[f] for f in want], dur, 0.15, 0.05)[0]


# ------------------------------------------------------------------ 6. end to end with boxes

E2E_MERGE = dict(MAX_GAP_SEC="0.5", PADDING_SEC="0.1", MIN_SAVINGS_PCT="5", VECTORS_NEEDED="1", CLUSTERS_NEEDED="1", CHUNK_DURATION_SEC="0.5")


@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    """persist_inputs.e2e_stream() as a .mtmv at 30 fps, a keep mask over the flash of frame 119, and the frames."""
    d = tmp_path_factory.mktemp("pipe_persist")
    p, mv, off, sd = pi.e2e_stream()
    frames = [mv[int(off[f]):int(off[f + 1])] if sd[f] else None for f in range(len(sd))]
    path = str(d / "e2e.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 90000, 30.0, len(sd) / 30.0, [3000 * f for f in range(len(sd))], frames)
    keep = np.ones((p.grid_h, p.grid_w), dtype=bool)
    keep[26:36, 76:88] = False                        # the flash in frame 119 (3 x 3 cells at (80, 30))
    mask = str(d / "flash119.mtkeep")
    zones.save_keep(mask, keep)
    pts = [(3000 * f) * (1.0 / 90000.0) for f in range(len(sd))]
    return path, mask, keep, p, frames, sd, pts


def test_scan_file_end_to_end_with_boxes(gpu_scanner_factory, e2e):
    """The event 120 .. 149 crosses the chunk border at frame 135.  --min-blob-cells 1 --min-run 3 --reach 1 keeps exactly
    frames 121 .. 149 (29 frames, one segment); without --reach the flash of frame 119 joins across the key frame 120
    (30); the scan itself finds 33 motion frames.  The run sweep equals the separate runs."""
    path, mask, keep, p, frames, sd, pts = e2e
    s = gpu_scanner_factory(p)
    env = tool_env(**E2E_MERGE)
    dur = len(sd) / 30.0
    n = len(sd)
    assert abs(pts[135] - 4.5) < 1e-9
    boxed = scan_file(env, path, "--min-blob-cells", 1, "--min-run", 3, "--reach", 1)
    assert boxed["timestamps"] == [pts[f] for f in pi.E2E_KEPT] and boxed["motion_frames"] == 29 and len(boxed["segments"]) == 1
    assert boxed["segments"] == merged(s, boxed["timestamps"], dur, 0.5, 0.1)[0]
    assert boxed["frames_before_persist"] == 33 and boxed["reach"] == 1 and boxed["min_run"] == 3 and boxed["chunks"] == 14
    loose = scan_file(env, path, "--min-blob-cells", 1, "--min-run", 3)
    assert loose["timestamps"] == [pts[f] for f in [119] + pi.E2E_KEPT] and loose["motion_frames"] == 30 and "reach" not in loose
    assert loose["frames_before_persist"] == 33
    # the run sweep: every level equals the separate run, level 1 the run without options
    plain = scan_file(env, path, "--min-blob-cells", 1)
    assert plain["motion_frames"] == 33 and "runs" not in plain
    sw = scan_file(env, path, "--min-blob-cells", 1, "--reach", 1, "--sweep-min-run", "1,2,3,5")
    assert [e["min_run"] for e in sw["sweep_min_run"]] == [1, 2, 3, 5] and sw["motion_frames"] == 33 and sw["min_run"] == 1
    flags = np.zeros(n, dtype=np.uint8)
    flags[list(pi.E2E_FLASHES) + pi.E2E_KEPT] = 1
    st = s.scan_blobs(m.FrameBatch.from_frames(list(frames)), 1)
    assert st["flags"].tolist() == flags.tolist()
    want = pmod.persist(flags, [0, n], sd, st["box"], min_run=1, max_dropout=0, reach=1)
    assert sw["runs"] == [[pts[f], int(want["run"][f])] for f in range(n)]
    for e in sw["sweep_min_run"]:
        one = plain if e["min_run"] == 1 else scan_file(env, path, "--min-blob-cells", 1, "--reach", 1, "--min-run", e["min_run"])
        for k in ("segments", "do_cut", "saved_pct", "n_timestamps"):
            assert e[k] == one[k], (e["min_run"], k)
    assert [e["n_timestamps"] for e in sw["sweep_min_run"]] == [33, 29, 29, 29]
    # the compensated blob mode, against the resident call and the model
    g = s.scan_gmc_blobs(m.FrameBatch.from_frames(list(frames)), _abi.GMC_DEFAULT_MAX_SHIFT, _abi.GMC_DEFAULT_MIN_SHARE_Q8, 1)
    want = pmod.persist(g["flags"], [0, n], sd, g["box"], min_run=3, max_dropout=0, reach=1)
    pair = scan_file(env, path, "--gmc-blobs", 1, "--min-run", 3, "--reach", 1)
    assert pair["timestamps"] == [pts[f] for f in range(n) if want["flags"][f]] and pair["motion_frames"] >= 29
    assert pair["frames_before_persist"] == int(np.count_nonzero(g["flags"]))
    # under a keep mask that covers the flash of frame 119: without --reach the event alone
    k = s.scan_blobs(m.FrameBatch.from_frames(list(frames)), 1, [0, n], zones.pack_keep(keep))
    assert k["flags"][119] == 0 and int(np.count_nonzero(k["flags"])) == 32
    want = pmod.persist(k["flags"], [0, n], sd, None, min_run=3, max_dropout=0)
    kept = scan_file(env, path, "--min-blob-cells", 1, "--min-run", 3, "--keep", mask)
    assert kept["timestamps"] == [pts[f] for f in range(n) if want["flags"][f]] == [pts[f] for f in pi.E2E_KEPT]
    assert kept["frames_before_persist"] == 32 and kept["ignored_cells"] == 120


def test_scan_file_refusals_name_both_sides(e2e):
    path = e2e[0]
    env = tool_env(**E2E_MERGE)
    exe = os.path.join(PKG, "mtgpu_scan_file")
    for args, words in ((["--min-run", "3", "--sweep", "2,3"], ("--min-run", "--sweep", "one persistence pass per level")),
                        (["--sweep-min-run", "2", "--sweep-blobs", "4"], ("--sweep-min-run", "--sweep-blobs")),
                        (["--min-run", "3", "--reach", "1"], ("--reach", "--min-blob-cells", "--gmc-blobs"))):
        out = subprocess.run([exe, path] + args, capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 2 and out.stdout == "" and all(w in out.stderr for w in words), out.stderr


# ------------------------------------------------------------------ 7. one worker pool, three videos

def test_next_video_inherits_neither_boxes_nor_persistence(e2e, tmp_path):
    """run_scan_pipeline three times on one pool of GpuBackends (tests/cpp/pipe_persist_two_videos.cpp): persistence with
    boxes, nothing, persistence without boxes."""
    path, _, _, p, frames, sd, pts = e2e
    exe = str(tmp_path / "pipe_persist_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_persist_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "2"], capture_output=True, text=True, env=tool_env(**E2E_MERGE), timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [dict(zip(ln.split()[0::2], ln.split()[1::2])) for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 3
    all_m = sorted(list(pi.E2E_FLASHES) + pi.E2E_KEPT)
    zc = m.LAYOUT_COMPACT8 | ZC
    want = [(pi.E2E_KEPT, 29, 33, str(zc | BX), 200, 33, 200), (all_m, 33, 0, str(zc), 0, 0, 0), ([119] + pi.E2E_KEPT, 30, 33, str(zc), 200, 0, 200)]
    for r, (kept, motion, before, layout, traced, boxed, nruns) in zip(runs, want):
        assert [float(t) for t in r["timestamps"].split(",")] == [pts[f] for f in kept], r["run"]
        assert int(r["motion_frames"]) == motion and int(r["before"]) == before and int(r["frames_scanned"]) == 200
        assert r["layouts"].split(",") == [layout] * 2, r["run"]
        assert (int(r["traced"]), int(r["boxed"]), int(r["runs"])) == (traced, boxed, nruns), r["run"]


# ------------------------------------------------------------------ 8. the example

def test_plain_c_pipe_boxes_example(gpu_scanner_factory, tmp_path):
    exe = str(tmp_path / "pipe_boxes_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_boxes_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    p, frames, pts = pp.example_case()
    s = gpu_scanner_factory(p)
    loose, boxed = pp.example_expected()
    assert (len(loose), len(boxed)) == (145, 58)
    nseg = [len(merged(s, [pts[f] for f in kept], pp.EX_FRAMES / pp.EX_FPS, 1.0, 0.5)[0]) for kept in (loose, boxed)]
    assert nseg == [2, 1]
    assert "MIN_RUN 3 without boxes:       motion frames %d, segments %d" % (len(loose), nseg[0]) in out.stdout
    assert "MIN_RUN 3 with boxes, reach 2: motion frames %d, segments %d" % (len(boxed), nseg[1]) in out.stdout
