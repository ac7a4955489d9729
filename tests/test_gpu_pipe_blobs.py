"""GPU tier (`-m gpu`): motion blobs carried through the pipe (include/mtgpu_pipe_blobs.h; csrc/blobs_kernels.hip, the
pipe form), the C++ host layer and mtgpu_scan_file.  Expected values: numbers derived by hand and the flood-fill model
(tests/pipe_blobs_inputs.py; both checked without a GPU by tests/test_pipe_blobs_host.py), and mtgpu_scan_frames_blobs /
the plain pipe on the same frames for the equality of the two paths.  Every comparison is exact."""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import pipe_blobs_inputs as pb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES
LAYOUTS = [rec | zc | ce for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC) for ce in (0, CE)]
LAYOUT_IDS = ["-".join([r] + z + c) for r in ("compact8", "aos40") for z in ([], ["zero-copy"]) for c in ([], ["centres"])]


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


def host_entry(s, frames, min_blob, keep=None):
    """mtgpu_scan_frames_blobs on the same frames as one stream -> {"flags", "centres", "largest"} lists."""
    b = m.FrameBatch.from_frames(list(frames))
    if keep is None:
        r = s.scan_blobs(b, min_blob)
    else:
        r = s.scan_blobs(b, min_blob, [0, len(frames)], zones.pack_keep(keep))
    return {k: r[k].tolist() for k in ("flags", "centres", "largest")}


# ------------------------------------------------------------------ 1. the rule bites

def test_the_rule_bites(gpu_scanner_factory):
    """Four separate pairs and one block of 2 x 4 both hold 8 centres: CLUSTERS_NEEDED 8 keeps both frames, a minimum
    blob size of 3 keeps only the block."""
    p, frames, hand = pb.bite_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2, centres=True)) as pipe:
        assert pipe.blobs is None
        assert run(pipe, frames) == ([1, 1], [8, 8])
        pipe.set_blobs(3, "centres")
        assert pipe.blobs == (3, "centres")
        assert run(pipe, frames) == ([0, 1], hand["centres"]) == ([0, 1], [8, 8])
        pipe.set_blobs(3, "largest")
        assert pipe.blobs == (3, "largest")
        assert run(pipe, frames) == ([0, 1], hand["largest"]) == ([0, 1], [2, 8])
        pipe.set_blobs(0, "centres")
        assert pipe.blobs is None
        assert run(pipe, frames) == ([1, 1], [8, 8])


def test_bad_arguments_change_nothing(gpu_scanner_factory):
    p, frames, hand = pb.bite_case()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2)) as pipe:                 # no MT_LAYOUT_CENTRES
        for args in ((-1, 0), (3, 2), (3, -1), (3, _abi.MT_PIPE_REPORT_LARGEST)):
            assert lib.mtgpu_pipe_set_blobs(pipe._pipe, *args) == _abi.MT_ERR_INVALID, args
            assert pipe.blobs is None
        assert "MT_LAYOUT_CENTRES" in lib.mtgpu_last_error().decode()
        with pytest.raises(ValueError):
            pipe.set_blobs(3, "boxes")
        assert run(pipe, frames)[0] == [1, 1]
        pipe.set_blobs(3)
        assert lib.mtgpu_pipe_set_blobs(pipe._pipe, -5, 0) == _abi.MT_ERR_INVALID and pipe.blobs == (3, "centres")
        assert run(pipe, frames)[0] == [0, 1]
        assert lib.mtgpu_pipe_set_blobs(pipe._pipe, 0, 77) == _abi.MT_OK and pipe.blobs is None      # report is ignored at 0
        n, r = ctypes.c_int32(7), ctypes.c_int(7)
        assert lib.mtgpu_pipe_blobs(pipe._pipe, ctypes.byref(n), ctypes.byref(r)) == 0 and (n.value, r.value) == (7, 7)
    with contextlib.closing(m.ScanPipe(s, 256, 4, 2, centres=True)) as pipe:
        pipe.set_blobs(4, "largest")
        assert lib.mtgpu_pipe_blobs(pipe._pipe, None, None) == 1
        pipe.set_blobs(0, "largest")
        pipe.set_blobs(2)                                                      # the report was reset to centres at 0
        assert pipe.blobs == (2, "centres")


# ------------------------------------------------------------------ 2. every layout and batch shape

@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_blob_pipe_in_every_layout_and_batch_shape(gpu_scanner_factory, layout):
    """14 ragged frames — without side data first, in the middle and last — in batches of 1 frame, of 4, of exactly
    cap_frames = 14 (then 7 + 7 exactly), and with a record capacity that makes every batch grow: flags and the reported
    count are the model's and mtgpu_scan_frames_blobs'."""
    p, frames = pb.shapes_case()
    s = gpu_scanner_factory(p)
    mo = pb.model(p, frames)
    want_f = pb.flags_of(p, mo, pb.MIN_BLOB)
    he = host_entry(s, frames, pb.MIN_BLOB)
    assert he == {"flags": want_f, "centres": mo["centres"], "largest": mo["largest"]}
    reports = ("centres", "largest") if layout & CE else ("centres",)
    for (max_rec, max_fr, nbuf) in [(256, 1, 1), (256, 4, 2), (512, 14, 2), (512, 7, 3), (8, 5, 2)]:
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout)) as pipe:
            for report in reports:
                pipe.set_blobs(pb.MIN_BLOB, report)
                got_f, got_c = run(pipe, frames)
                assert got_f == want_f, (max_rec, max_fr, nbuf, report)
                assert got_c == (mo[report] if layout & CE else None), (max_rec, max_fr, nbuf, report)
    # one frame through a pipe of one batch
    with contextlib.closing(m.ScanPipe(s, 256, 1, 1, layout=layout)) as pipe:
        pipe.set_blobs(pb.MIN_BLOB, reports[-1])
        for i in (1, 2, 0):
            got_f, got_c = run(pipe, frames[i:i + 1])
            assert got_f == want_f[i:i + 1] and got_c == (mo[reports[-1]][i:i + 1] if layout & CE else None)


# ------------------------------------------------------------------ 3. the seam, the largest union

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40], ids=["compact8-zero-copy", "aos40"])
def test_word_seam_and_the_frame_filling_blob(gpu_scanner_factory, layout):
    p, frames, hand = pb.seam_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
        pipe.set_blobs(5, "largest")
        assert run(pipe, frames) == ([1, 1, 1, 0], hand["largest"])
        pipe.set_blobs(5, "centres")
        assert run(pipe, frames) == ([1, 1, 1, 0], hand["centres"])
    assert host_entry(s, frames, 5) == {"flags": [1, 1, 1, 0], "centres": hand["centres"], "largest": hand["largest"]}
    p, frames, hand = pb.vn0_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
        pipe.set_blobs(118 * 68, "largest")
        assert run(pipe, frames) == ([1], [118 * 68])
        pipe.set_blobs(118 * 68 + 1, "centres")
        assert run(pipe, frames) == ([0], [118 * 68])


# ------------------------------------------------------------------ 4. mask and blobs together

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40], ids=["compact8-zero-copy", "aos40"])
def test_mask_and_blobs_commute(gpu_scanner_factory, layout):
    """The cleared column splits each block: largest 8 -> 4 (and 2), 10 -> 4 + 4.  set_keep then set_blobs, and the
    reverse, give the same pipe; set_keep(None) afterwards leaves the unmasked blob scan."""
    p, frames, keep, plain, masked = pb.mask_case()
    s = gpu_scanner_factory(p)
    mb = pb.MASK_MIN_BLOB
    he = host_entry(s, frames, mb, keep)
    assert he == {"flags": [0, 0], "centres": masked["centres"], "largest": masked["largest"]}
    results = []
    for order in ("keep-first", "blobs-first"):
        with contextlib.closing(m.ScanPipe(s, 64, 4, 2, layout=layout, centres=True)) as pipe:
            if order == "keep-first":
                pipe.set_keep(keep)
                pipe.set_blobs(mb, "largest")
            else:
                pipe.set_blobs(mb, "largest")
                pipe.set_keep(keep)
            assert pipe.has_keep and pipe.blobs == (mb, "largest")
            a = run(pipe, frames)
            pipe.set_blobs(mb, "centres")
            b = run(pipe, frames)
            pipe.set_blobs(1, "largest")                       # min_blob_cells 1: the masked scan's flags
            c = run(pipe, frames)
            pipe.set_blobs(mb, "largest")
            pipe.set_keep(None)
            assert not pipe.has_keep and pipe.blobs == (mb, "largest")
            d = run(pipe, frames)
            pipe.set_keep(keep)
            pipe.set_blobs(0)                                  # the masked scan alone, as before this feature
            assert pipe.has_keep and pipe.blobs is None
            e = run(pipe, frames)
            results.append((a, b, c, d, e))
    assert results[0] == results[1]
    a, b, c, d, e = results[0]
    assert a == ([0, 0], masked["largest"]) == ([0, 0], [4, 4])
    assert b == ([0, 0], masked["centres"]) == ([0, 0], [6, 8])
    assert c == ([0, 1], masked["largest"])
    assert d == ([1, 1], plain["largest"]) == ([1, 1], [8, 10])
    assert e == ([0, 1], masked["centres"])


# ------------------------------------------------------------------ 5. stale results in the pinned block

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", ["centres", "largest"])
def test_no_stale_results_in_a_reused_pinned_block(gpu_scanner_factory, layout, report):
    """n_buffers = 1, zero-copy: batch 1 leaves flag 1 / count 12 in every slot of the pinned block; batch 2 goes into
    the same slots and every flag and count must read the new value — from the store behind the labelling passes, from
    the early-exit store and from the planning kernel."""
    p, one, two, h1, h2 = pb.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 256, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_blobs(pb.MIN_BLOB, report)
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, two) == (h2["flags"], h2[report])
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, list(reversed(two))) == ([0, 0, 0], list(reversed(h2[report])))


# ------------------------------------------------------------------ 6. one pipe, two recordings, and busy

def test_one_pipe_two_recordings_and_busy(gpu_scanner_factory):
    p, frames = pb.shapes_case()
    s = gpu_scanner_factory(p)
    mo = pb.model(p, frames)
    at3, at9 = (pb.flags_of(p, mo, 3), mo["centres"]), (pb.flags_of(p, mo, 9), mo["largest"])
    plain = (pb.flags_of(p, mo, 1), mo["centres"])
    assert at3[0] != at9[0] != plain[0]
    n = len(frames)
    with contextlib.closing(m.ScanPipe(s, 256, 4, 3, centres=True)) as pipe:
        pipe.set_blobs(3, "centres")
        assert run(pipe, frames) == at3
        # a batch being filled: MT_ERR_BUSY, and the run that follows still uses the old setting
        feed_all(pipe, frames[:3])
        for args in ((9, "largest"), (0, "centres")):
            with pytest.raises(m.MtgpuError) as e:
                pipe.set_blobs(*args)
            assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value) and pipe.blobs == (3, "centres")
        for i in range(3, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == at3
        # a batch in flight: the same
        feed_all(pipe, frames[:6])                             # 4 submitted, 2 being filled
        pipe._submit()
        assert pipe._cur is None and pipe._inflight >= 1
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_blobs(9, "largest")
        assert e.value.code == _abi.MT_ERR_BUSY and "in flight" in str(e.value) and pipe.blobs == (3, "centres")
        for i in range(6, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == at3
        # after collect the call succeeds and applies: the next recording
        pipe.set_blobs(9, "largest")
        assert run(pipe, frames) == at9
        pipe.set_blobs(0)
        assert run(pipe, frames) == plain


# ------------------------------------------------------------------ 7. the 4K grid

def test_4k_grid(gpu_scanner_factory):
    p, frames = pb.uhd_case()
    s = gpu_scanner_factory(p)
    mo = pb.model(p, frames)
    want_f = pb.flags_of(p, mo, 3)
    assert want_f == [1, 0, 1, 0, 0, 1]
    assert host_entry(s, frames, 3) == {"flags": want_f, "centres": mo["centres"], "largest": mo["largest"]}
    for layout in (m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC):
        with contextlib.closing(m.ScanPipe(s, 2048, 6, 2, layout=layout, centres=True)) as pipe:
            pipe.set_blobs(3, "largest")
            assert run(pipe, frames) == (want_f, mo["largest"])
            pipe.set_blobs(3, "centres")
            assert run(pipe, frames) == (want_f, mo["centres"])


# ------------------------------------------------------------------ 8. a grid without a blob form

def test_grid_without_a_blob_form(gpu_scanner_factory):
    """960 x 540 cells: set_blobs is MT_ERR_UNSUPPORTED with the grid named, the setting stays off and the pipe goes on
    scanning plainly."""
    from mvtrim_amd import synth
    p = m.ScanParams.from_config(3840, 2160, **pb.FINE_KW)
    s = gpu_scanner_factory(p)
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    want = s.check_frames(m.FrameBatch.from_frames(frames)).tolist()
    assert want == [0, 1, 1]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_blobs(3)
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.blobs is None and m.load_library().mtgpu_pipe_blobs(pipe._pipe, None, None) == 0
        assert run(pipe, frames)[0] == want


# ------------------------------------------------------------------ 9. sweep from one pass

def test_collected_largest_through_the_sweep_is_the_flags_through_the_merge(gpu_scanner_factory):
    """One decode pass with MT_PIPE_REPORT_LARGEST; its counts through mtgpu_sweep_streams_device at levels 2, 4, 8 (all
    >= CLUSTERS_NEEDED 2) == the pipe's flags at min_blob_cells = L through mtgpu_merge_streams_device, bit patterns
    compared."""
    import torch
    p, frames, pts, _ = pb.recording_case()
    s = gpu_scanner_factory(p)
    CAP, levels = 16, [2, 4, 8]
    d_pts = torch.tensor(pts, dtype=torch.float64).cuda()
    d_soff = torch.tensor([0, len(frames)], dtype=torch.int64).cuda()
    mp = m.MergeParams(duration=pb.REC_FRAMES / pb.REC_FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    d_mp = torch.from_numpy(mp.to_record().view(np.uint8).copy()).cuda()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)        # noqa: E731
    with contextlib.closing(m.ScanPipe(s, 512, 10, 3, centres=True)) as pipe:
        pipe.set_blobs(1, "largest")
        _, largest = run(pipe, frames, pts)
        assert largest == pb.REC_LARGEST
        d_largest = torch.tensor(largest, dtype=torch.int32).cuda()
        sseg, sres = s.sweep_streams_device(d_largest, d_pts, d_soff, d_mp, levels, seg_cap=CAP)
        torch.cuda.synchronize()
        kept = []
        for li, lv in enumerate(levels):
            pipe.set_blobs(lv, "largest")
            fl, again = run(pipe, frames, pts)
            assert again == largest
            seg, r8 = s.merge_streams_device(torch.tensor(fl, dtype=torch.uint8).cuda(), d_pts, d_soff, d_mp, seg_cap=CAP)
            torch.cuda.synchronize()
            assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg.cpu().numpy())), lv
            assert np.array_equal(sres[li].cpu().numpy(), r8.cpu().numpy()), lv
            kept.append(sum(fl))
    assert kept == [48, 24, 12]


# ------------------------------------------------------------------ 10. launch scratch and profiling

def test_blob_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    p, one, two, h1, h2 = pb.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 256, 1, 2, centres=True)) as pipe:
        pipe.set_blobs(pb.MIN_BLOB, "largest")
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, one) == (h1["flags"], h1["largest"])          # three batches of one frame
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


# ------------------------------------------------------------------ 11. mtgpu_scan_file

MERGE_ENV = dict(MAX_GAP_SEC="0.1", PADDING_SEC="0.04", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="25",
                 VECTORS_NEEDED="1")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 48-frame recording as a .mtmv file, its mask as a .mtkeep file."""
    d = tmp_path_factory.mktemp("pipe_blobs")
    p, frames, pts, keep = pb.recording_case()
    path = str(d / "rec.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, pb.REC_FPS, pb.REC_FRAMES / pb.REC_FPS, list(range(pb.REC_FRAMES)), list(frames))
    mask = str(d / "col44.mtkeep")
    zones.save_keep(mask, keep)
    env = dict(os.environ, **MERGE_ENV)
    for k in ("CLUSTERS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, env


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=pb.REC_FRAMES / pb.REC_FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def scan_file(env, path, *args):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2"] + list(args), capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def test_scan_file_min_blob_cells_and_sweep_blobs(gpu_scanner_factory, recording):
    path, mask, env = recording
    p, frames, pts, keep = pb.recording_case()
    s = gpu_scanner_factory(p)
    plain = scan_file(env, path)
    assert plain["motion_frames"] == 48 and "largest" not in plain and "sweep_blobs" not in plain
    by_level = {}
    for keep_args, kp in (([], None), (["--keep", mask], keep)):
        mo = pb.model(p, frames, kp)
        for lv in (4, 8):
            fl = pb.flags_of(p, mo, lv)
            want_seg, want_res = python_segments(s, fl, pts)
            r = scan_file(env, path, "--min-blob-cells", str(lv), *keep_args)
            assert r["motion_frames"] == sum(fl) and r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"], (lv, keep_args)
            assert r["frames_scanned"] == 48 and ("ignored_cells" in r) == bool(keep_args)
            by_level[(lv, bool(keep_args))] = r
    assert [by_level[k]["motion_frames"] for k in ((4, False), (8, False), (4, True), (8, True))] == [24, 12, 24, 0]
    assert scan_file(env, path, "--min-blob-cells", "0")["segments"] == plain["segments"]
    # one pass, every level: the per-level entries are the separate runs
    for keep_args, largest in (([], pb.REC_LARGEST), (["--keep", mask], pb.REC_LARGEST_MASKED)):
        r = scan_file(env, path, "--sweep-blobs", "2,4,8", *keep_args)
        assert [n for _, n in r["largest"]] == largest and [t for t, _ in r["largest"]] == list(pts)
        assert r["segments"] == plain["segments"] and "centres" not in r and "sweep" not in r
        assert [e["min_blob_cells"] for e in r["sweep_blobs"]] == [2, 4, 8]
        assert r["sweep_blobs"][0]["segments"] == plain["segments"]
        for e in r["sweep_blobs"][1:]:
            sep = by_level[(e["min_blob_cells"], bool(keep_args))]
            assert e["segments"] == sep["segments"] and e["do_cut"] == sep["do_cut"] and e["saved_pct"] == sep["saved_pct"]
            assert e["n_timestamps"] == sep["n_timestamps"]
    # --sweep-blobs next to --min-blob-cells: the job's own segments follow the rule, the sweep is unchanged
    r = scan_file(env, path, "--sweep-blobs", "4", "--min-blob-cells", "8")
    assert r["segments"] == by_level[(8, False)]["segments"] and r["sweep_blobs"][0]["segments"] == by_level[(4, False)]["segments"]


# ------------------------------------------------------------------ 12. one worker pool, several videos

def test_next_video_does_not_inherit_the_blob_setting(recording, tmp_path):
    """run_scan_pipeline three times on one pool of GpuBackends (tests/cpp/pipe_blobs_two_videos.cpp): min_blob_cells 4,
    none, min_blob_cells 4 with the sweep.  The second video's flags are the plain scan's and its pipes carry no setting."""
    path, _, env = recording
    p, frames, pts, _ = pb.recording_case()
    exe = str(tmp_path / "pipe_blobs_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_blobs_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "4", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 3
    mo = pb.model(p, frames)
    for i, r in enumerate(runs):
        kv = dict(zip(r[0::2], r[1::2]))
        w = pb.flags_of(p, mo, 4 if i != 1 else 1)
        ts = [float(t) for t in kv.get("timestamps", "").split(",") if t]
        assert ts == [pts[f] for f in range(pb.REC_FRAMES) if w[f]], i
        assert int(kv["motion_frames"]) == sum(w) == (48 if i == 1 else 24) and int(kv["frames_scanned"]) == 48
        assert kv["blobs"].split(",") == [("4", "0", "4L")[i]] * 2
        assert int(kv["sweep_frames"]) == (24 if i == 2 else -1)


# ------------------------------------------------------------------ 13. the example

def test_plain_c_pipe_blobs_example(tmp_path):
    exe = str(tmp_path / "pipe_blobs_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_blobs_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "CLUSTERS_NEEDED 8 alone:  motion frames 58, segments 2" in out.stdout
    assert "with MIN_BLOB_CELLS 3:    motion frames 29, segments 1" in out.stdout
