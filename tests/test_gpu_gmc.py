"""GPU tier (`-m gpu`): global-motion compensation — the centre scan on the residuals of each frame's dominant vector
(include/mtgpu_gmc.h, csrc/gmc_kernels.hip).

Expected values: numbers written out by hand in tests/gmc_inputs.py; mtgpu_scan_centres_device (existing code) for
max_shift 0 and vectors_needed 0 (consequences A and D of the header); the unchanged oracle on records whose src has the
applied vector added (consequence C); the kernel against itself on translated records (consequence B); and the numpy
restatement of tests/gmc_model.py for the estimate's own outputs.  tests/test_gmc_host.py holds all of them against
each other without a GPU.  Every comparison is exact; outputs are pre-filled with junk: every element must be written by
the call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, gmc, synth

import derived_edge_inputs as dei
import gmc_inputs as gi
import gmc_model as gm
import oracle_binding as ob
from golden_cases import load_hand_cases
from scan_checks import assert_counts_equal, device_centres_of, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG = -7, 9


def device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact, stream=None):
    """Through mtgpu_scan_gmc_device into junk-filled outputs -> (flags uint8, centres uint32, info GMC_INFO_DTYPE) on
    the host."""
    import torch
    n = d_off.numel() - 1
    fl = torch.full((n,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    inf = torch.full((n, 5), JUNK, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.scan_gmc_device(d_rec, d_off, d_sd, ms, q8, compact=compact, flags=fl, centres=ce, info=inf, stream=stream)
    torch.cuda.synchronize()
    return fl.cpu().numpy(), ce.cpu().numpy().view(np.uint32), inf.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE)


def gmc_both_layouts(s, mv, off, sd, ms, q8, what):
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        yield (f"{what}, {'compact' if compact else '40-byte'}",) + device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact)


def assert_info_equal(got, want_rows, what):
    got_rows = gi.info_rows(got)
    want_rows = np.asarray(want_rows, dtype=np.int64).reshape(-1, 7)
    bad = np.flatnonzero((got_rows != want_rows).any(axis=1))
    assert bad.size == 0, (f"{what}: info of {bad.size} frames differs, first {bad[:4].tolist()}: want {want_rows[bad[:4]].tolist()} "
                           f"got {got_rows[bad[:4]].tolist()} (fields {gi.INFO_FIELDS})")


# ------------------------------------------------------------------ 1. the hand cases

def test_hand_cases(gpu_scanner_factory):
    """Every case of gmc_inputs.HAND on the 8 x 6 grid, grouped by what a call shares, each followed by a frame without
    side data that owns records; both layouts and the host entry point."""
    seen = 0
    for (thr, margin, ms, q8), names, mv, off, sd, want_c, want_i, plain in gi.hand_batches():
        s = gpu_scanner_factory(gi.hand_params(thr, margin))
        for label, fl, ce, info in gmc_both_layouts(s, mv, off, sd, ms, q8, "/".join(names)):
            assert_counts_equal(ce, want_c, label, got_f=fl, want_f=(want_c >= 1).astype(np.uint8))
            assert_info_equal(info, want_i, label)
        hf, hc, hi = s.scan_gmc(m.FrameBatch(mv, off, None, sd), ms, q8)
        assert hc.dtype == np.uint32 and hi.dtype == _abi.GMC_INFO_DTYPE
        assert_counts_equal(hc, want_c, "host entry " + "/".join(names), got_f=hf, want_f=(want_c >= 1).astype(np.uint8))
        assert_info_equal(hi, want_i, "host entry " + "/".join(names))
        # the plain scan of the same frames, by hand too
        d_rec, d_off, d_sd = to_device(mv, off, sd, True)
        assert_counts_equal(device_centres_of(s, d_rec, d_off, d_sd, True)[1], plain, "plain scan " + "/".join(names))
        seen += len(names)
    assert seen == len(gi.HAND) == 17


# ------------------------------------------------------------------ 2. consequence A: max_shift 0 is the centre scan

def assert_is_the_centre_scan(s, mv, off, sd, ms, q8, what, hand=None):
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        want_f, want_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact)
        label = f"{what}, {'compact' if compact else '40-byte'}"
        assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
        if hand is not None:
            assert_counts_equal(ce, hand, label + " against the hand values")
        if ms == 0:
            assert not info["gx"].any() and not info["gy"].any() and not info["mode_x"].any() and not info["mode_y"].any(), label
    return want_c, info


def test_hand_derived_check_frame_cases_with_max_shift_0(gpu_scanner_factory):
    """The 30 hand-derived check_frame cases, each alone, under its own VECTORS_NEEDED, 0 and 255."""
    _, cases = load_hand_cases()
    assert len(cases) == 30
    scanners = {}
    nonzero = 0
    for name, kw, case in cases:
        mv, off, sd, hand = dei.hand_case_batch(case)
        for vn in (kw["vectors_needed"], 0, 255):
            key = tuple(sorted(dict(kw, vectors_needed=vn).items()))
            if key not in scanners:
                scanners[key] = gpu_scanner_factory(m.ScanParams.from_config(**dict(key)))
            got, _ = assert_is_the_centre_scan(scanners[key], mv, off, sd, 0, 128, f"{name} vn {vn}",
                                               [hand] if vn == kw["vectors_needed"] else None)
            nonzero += int(got[0] > 0)
    assert nonzero == 45                                             # as for the zones: the oracle's counts of the same 90 scans


@pytest.mark.parametrize("vn", [0, 1, 2])
def test_random_frames_with_max_shift_0_and_with_vectors_needed_0(gpu_scanner_factory, vn):
    """synth.random_frames (ragged, extreme coordinates, frames without side data): max_shift 0 is the centre scan for
    every vn (A); vn == 0 is the centre scan for every max_shift (D); n_in is the number of records the bounds test of
    :262 lets through."""
    rng = np.random.RandomState(100 + vn)
    mv, off, sd = synth.random_frames(rng, 40, 3000, 1920, 1080)
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=vn)
    s = gpu_scanner_factory(p)
    want_c, info = assert_is_the_centre_scan(s, mv, off, sd, 0, 128, f"random frames vn {vn}")
    assert vn == 0 or int((want_c > 0).sum()) >= 10
    want_n = [int(gm.counted(p, mv[int(off[f]):int(off[f + 1])]).sum()) if sd[f] else 0 for f in range(40)]
    assert info["n_in"].tolist() == want_n and max(want_n) > 1000
    if vn == 0:
        _, info = assert_is_the_centre_scan(s, mv, off, sd, 16, 0, "random frames vn 0, max_shift 16")
        assert info["gx"].any() and info["gy"].any()              # something was subtracted, and it changed nothing


# ------------------------------------------------------------------ 3. consequences B and C on random pans

@pytest.mark.parametrize("vn", [1, 2])
def test_random_pans_against_the_oracle_and_under_translation(gpu_scanner_factory, vn):
    """gi.pan_batch(): record counts 0, 1, 15, 16, 17, 4095, 4096, 4097 back to back (frame starts off the 128-byte
    lines), every fifth frame without side data.  C: centres == the oracle's plain count of the records with (gx, gy)
    added to every src; info == the numpy model's.  B: with (a, b) added to every src of a frame whose axes are both
    supported, (gx, gy) becomes (gx - a, gy - b) and centres stays."""
    mv, off, sd, pans, shifts = gi.pan_batch()
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=vn)
    s = gpu_scanner_factory(p)
    ms, q8 = gi.PAN_MAX_SHIFT, 128
    _, model_c, model_i = gm.gmc_batch(p, mv, off, sd, ms, q8)
    supported = (model_i["gx"] == model_i["mode_x"]) & (model_i["gy"] == model_i["mode_y"]) & (sd != 0) & (model_i["n_in"] > 0)
    supported &= (model_i["n_x"].astype(np.int64) * 256 >= q8 * model_i["n_in"].astype(np.int64))
    supported &= (model_i["n_y"].astype(np.int64) * 256 >= q8 * model_i["n_in"].astype(np.int64))
    assert int(supported.sum()) >= 8
    a = np.where(supported, shifts[:, 0], 0)
    b = np.where(supported, shifts[:, 1], 0)
    assert (np.abs(model_i["mode_x"].astype(np.int64) - a) <= ms).all() and (np.abs(model_i["mode_y"].astype(np.int64) - b) <= ms).all()
    moved = gm.shift_src(mv, off, a, b)
    assert moved is not None
    for compact in (False, True):
        label = f"random pans vn {vn}, {'compact' if compact else '40-byte'}"
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        if not compact:
            assert sum(1 for f in range(len(off) - 1) if (int(off[f]) * 40) % 128) >= 6
        fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact)
        assert_info_equal(info, gi.info_rows(model_i), label)
        back = gm.shift_src(mv, off, info["gx"], info["gy"])
        want_f, want_c = ob.scan_centres(p, back, off, sd, nthreads=4)
        assert_counts_equal(ce, want_c, label + " (C)", got_f=fl, want_f=want_f)
        big = np.diff(off.astype(np.int64)) >= 4095
        assert int((big & (sd != 0)).sum()) >= 5 and (ce[big & (sd != 0)] > 0).all()
        # B
        d_rec2, _, _ = to_device(moved, off, sd, compact)
        fl2, ce2, info2 = device_gmc(s, d_rec2, d_off, d_sd, ms, q8, compact)
        assert_counts_equal(ce2, ce, label + " (B)", got_f=fl2, want_f=fl)
        assert (info2["gx"].astype(np.int64) == info["gx"].astype(np.int64) - a).all(), label
        assert (info2["gy"].astype(np.int64) == info["gy"].astype(np.int64) - b).all(), label
        assert info2["n_in"].tolist() == info["n_in"].tolist() and info2["n_x"].tolist() == info["n_x"].tolist()


# ------------------------------------------------------------------ 4. a residual beyond 32 bits

@pytest.mark.parametrize("thr,want", gi.BIG_THRESHOLDS)
def test_residual_square_beyond_32_bits(gpu_scanner_factory, thr, want):
    """gi.big_frame(): a residual of 65 662, its square 4 311 498 244; thresholds on both sides; from exact integers."""
    mv, off, sd = gi.big_frame()
    s = gpu_scanner_factory(m.ScanParams.from_config(32768, 32768, mv_threshold_sq=thr, vectors_needed=1, clusters_needed=1, **dei.BIG_KW))
    for label, fl, ce, info in gmc_both_layouts(s, mv, off, sd, 127, 128, f"threshold {thr}"):
        assert_counts_equal(ce, [want], label, got_f=fl, want_f=[want])
        assert_info_equal(info, [gi.BIG_INFO], label)


# ------------------------------------------------------------------ 5. the largest layout

def test_one_frame_on_240x135_without_margin(gpu_scanner_factory):
    """The largest layout the preview accepts (137 984 bytes of LDS): a pan of (7, -3) over every cell of the grid, the
    corners and the last row included, and a 3 x 2 object; against the model and the oracle (C)."""
    p = m.ScanParams.from_config(3840, 2160, vertical_mask=0.0, vectors_needed=1)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (240, 135, 0) and m.gmc_preview(p)["lds_bytes"] == 137984
    obj = {(x, y) for x in (237, 238, 239) for y in (133, 134)} | {(100, 70), (101, 70)}
    cells = [(x, y, 1, 16, -3) if (x, y) in obj else (x, y, 1, 7, -3) for y in range(135) for x in range(240)]
    mv = dei.voters(cells, 4)
    mv = mv[np.random.RandomState(3).permutation(len(mv))]
    off, sd = np.array([0, len(mv)], dtype=np.uint64), np.ones(1, dtype=np.uint8)
    c, info = gm.gmc_frame(p, mv, 16, 128)
    # by hand: residual 9 in the object's cells; (237, 133), (238, 133), (237, 134), (238, 134), (100, 70), (101, 70)
    # are centres, column 239 never is
    assert c == 6 and (info["gx"], info["gy"], info["n_in"], info["n_x"]) == (7, -3, 32400, 32392)
    assert int(ob.scan_centres(p, gm.shift_src(mv, off, [7], [-3]), off, sd)[1][0]) == 6
    s = gpu_scanner_factory(p)
    for label, fl, ce, got in gmc_both_layouts(s, mv, off, sd, 16, 128, "240x135"):
        assert_counts_equal(ce, [6], label, got_f=fl, want_f=[1])
        assert_info_equal(got, [[7, -3, 7, -3, 32400, 32392, 32400]], label)


# ------------------------------------------------------------------ 6. exact writes

def test_exact_writes(gpu_scanner_factory):
    """Canaries on both sides of every output, each output NULL in turn and in pairs, all three NULL, n_frames == 0,
    failing calls, and a non-default stream."""
    import torch
    mv, off, sd, pans, shifts = gi.pan_batch()
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1)
    ms, q8 = gi.PAN_MAX_SHIFT, 128
    want_f, want_c, want_i = gm.gmc_batch(p, mv, off, sd, ms, q8)
    want = {"flags": want_f, "centres": want_c, "info": gi.info_rows(want_i)}
    s = gpu_scanner_factory(p)
    lib = s._lib
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    F, PAD = len(off) - 1, 64
    NAMES = ("flags", "centres", "info")
    WIDTH = {"flags": 1, "centres": 1, "info": 5}

    def buffers():
        b = {"flags": torch.full((F + 2 * PAD,), JUNK_FLAG, dtype=torch.uint8, device="cuda"),
             "centres": torch.full((F + 2 * PAD,), JUNK, dtype=torch.int32, device="cuda"),
             "info": torch.full(((F + 2 * PAD) * 5,), JUNK, dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        return b

    def run(names, n_frames=F, rb=8, stream=None, ctx=None, over=None, ms_=ms, q8_=q8):
        b = buffers()
        ptr = {n: (b[n][PAD * WIDTH[n]:].data_ptr() if n in names else None) for n in NAMES}
        ptr.update(over or {})
        rc = lib.mtgpu_scan_gmc_device((ctx or s)._ctx, d_rec.data_ptr(), rb, len(mv), d_off.data_ptr(), d_sd.data_ptr(), n_frames,
                                       ms_, q8_, ptr["flags"], ptr["centres"], ptr["info"], stream)
        torch.cuda.synchronize()
        return rc, {n: t.cpu().numpy() for n, t in b.items()}

    def untouched(raw, names=NAMES):
        return all((raw[n] == (JUNK_FLAG if n == "flags" else JUNK)).all() for n in names)

    def check(raw, names):
        for n in NAMES:
            junk, w = (JUNK_FLAG if n == "flags" else JUNK), WIDTH[n]
            assert (raw[n][:PAD * w] == junk).all() and (raw[n][(PAD + F) * w:] == junk).all(), (names, n)
            if n in names:
                got = raw[n][PAD * w:(PAD + F) * w]
                if n == "info":
                    got = gi.info_rows(np.ascontiguousarray(got).view(_abi.GMC_INFO_DTYPE))
                elif n == "centres":
                    got = got.view(np.uint32)
                assert np.array_equal(got, want[n]), (names, n)
            else:
                assert untouched(raw, (n,)), (names, n)

    for names in [NAMES, ("flags", "centres"), ("flags", "info"), ("centres", "info"), ("flags",), ("centres",), ("info",)]:
        rc, raw = run(names)
        assert rc == _abi.MT_OK, (names, lib.mtgpu_last_error())
        check(raw, names)
    # all three NULL
    rc, raw = run(())
    assert rc == _abi.MT_ERR_INVALID and "all NULL" in lib.mtgpu_last_error().decode() and untouched(raw)
    # n_frames == 0: MT_OK, nothing written
    rc, raw = run(NAMES, n_frames=0)
    assert rc == _abi.MT_OK and untouched(raw)
    hf, hc, hi = s.scan_gmc(m.FrameBatch(mv[:0], off[:1], None, None))
    assert len(hf) == len(hc) == len(hi) == 0
    # failing calls touch no byte: rec_bytes, the two settings, an output in pinned host memory, an unsupported grid
    for rb in (0, 16, 41):
        rc, raw = run(NAMES, rb=rb)
        assert rc == _abi.MT_ERR_INVALID and "rec_bytes" in lib.mtgpu_last_error().decode() and untouched(raw)
    rc, raw = run(NAMES, ms_=128)
    assert rc == _abi.MT_ERR_INVALID and "max_shift" in lib.mtgpu_last_error().decode() and untouched(raw)
    rc, raw = run(NAMES, q8_=257)
    assert rc == _abi.MT_ERR_INVALID and "min_share_q8" in lib.mtgpu_last_error().decode() and untouched(raw)
    rc, raw = run(NAMES, over={"info": d_rec.data_ptr() + 2})
    assert rc == _abi.MT_ERR_INVALID and "d_info must be 4-byte aligned" in lib.mtgpu_last_error().decode() and untouched(raw)
    pinned = torch.full((F * 5,), JUNK, dtype=torch.int32).pin_memory()
    for name in NAMES:
        rc, raw = run(NAMES, over={name: pinned.data_ptr()})
        assert rc == _abi.MT_ERR_INVALID and ("d_" + name + " is not memory of device") in lib.mtgpu_last_error().decode()
        assert untouched(raw) and int((pinned != JUNK).sum()) == 0
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    rc, raw = run(NAMES, ctx=big)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in lib.mtgpu_last_error().decode() and untouched(raw)
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_gmc(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # a non-default stream
    st = torch.cuda.Stream()
    rc, raw = run(NAMES, stream=st.cuda_stream)
    assert rc == _abi.MT_OK
    check(raw, NAMES)


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    mv, off, sd, pans, shifts = gi.pan_batch()
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=2)
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    s.profile(True)
    try:
        s.profile_read()
        fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, gi.PAN_MAX_SHIFT, 128, False)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert ce.tolist() == gm.gmc_batch(p, mv, off, sd, gi.PAN_MAX_SHIFT, 128)[1].tolist()


# ------------------------------------------------------------------ 7. the example and the command

def test_plain_c_gmc_example(tmp_path):
    """examples/gmc_example.c: a swaying camera from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "gmc_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "gmc_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame 13: 8024 centres without compensation, 3 with, applied vector (5, 0)" in out.stdout
    assert "motion frames: 44 of 60 without compensation, 10 with; 40 frames compensated" in out.stdout


def test_end_to_end_command_on_a_shaken_stream(tmp_path):
    """A 640 x 368 stream of 40 frames with a shaking camera (synth.StreamSpec.shake = 6) and one scripted event in
    frames 12 .. 19, written as .mtmv; `python -m mvtrim_amd.gmc --json` in a fresh child process.  The background of
    the generator is U{-1, 0, 1} per axis: its mode holds a third of the records, so --min-share 0.3 (the largest of
    three bins that share 828 of 840 analysed records holds at least 276 > 0.3 x 840).  Whatever of the three is picked,
    a background residual is at most 2 per axis, 8 < 16; the event's is at least 8 on x."""
    F = 40
    spec = synth.StreamSpec(640, 368, 16, 1, fps=25.0, gop=10, seed=5, salt_p=0.0, oob_p=0.0, shake=6,
                            events=[synth.Event(12, 20, 10, 8, 4, 3, 9, 2)])
    frames = [synth.gen_frame(spec, f) for f in range(F)]
    path = str(tmp_path / "shaken.mtmv")
    m.mvfile.write_mtmv(path, 640, 368, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.gmc", path, "--json", "--vectors-needed", "1", "--min-share", "0.3",
                          "--max-gap-sec", "0.2", "--padding-sec", "0.04", "--min-savings-pct", "5"],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert (doc["grid_w"], doc["grid_h"], doc["frames"], doc["max_shift"], doc["min_share_q8"]) == (40, 23, F, 16, 77)
    assert doc["with_gmc"]["kept"] == list(range(12, 20))                 # exactly the scripted event's frames
    assert doc["with_gmc"]["motion_frames"] == 8 < doc["without_gmc"]["motion_frames"]
    assert set(range(12, 20)) <= set(doc["without_gmc"]["kept"])
    assert doc["with_gmc"]["segments"] == 1 and doc["with_gmc"]["frames_kept"] == 8
    # the plain scan keeps exactly the frames whose camera displacement alone passes the threshold somewhere, and the
    # event's: a frame whose shake stays below 3 per axis cannot reach 16 with the background's +-1
    cams = [synth.camera_shift(spec, f) for f in range(F)]
    for f in range(F):
        if frames[f] is not None and f not in range(12, 20) and max(abs(cams[f][0]), abs(cams[f][1])) >= 5:
            assert f in doc["without_gmc"]["kept"], f
    assert 0.5 < doc["compensated_share"] <= 1.0
    # the applied vectors are the camera's, up to the background's +-1
    from mvtrim_amd import tune
    batch, fpts, hdr = tune.load(path)
    p = m.ScanParams.from_config(640, 368, vectors_needed=1)
    _, _, info = gm.gmc_batch(p, np.ascontiguousarray(batch.mv, dtype=m.MV_DTYPE), batch.frame_off, batch.has_sd, 16, 77)
    for f in range(F):
        if frames[f] is not None:
            assert abs(int(info["gx"][f]) + cams[f][0]) <= 1 and abs(int(info["gy"][f]) + cams[f][1]) <= 1, f
    top = doc["vectors"][0]
    assert top[2] == int(((info["gx"] == top[0]) & (info["gy"] == top[1]) & (np.asarray(batch.has_sd) != 0)).sum())


# ------------------------------------------------------------------ 8. the pick across lanes and trips

def test_pick_across_lanes_and_trips(gpu_scanner_factory):
    """gi.LANES, max_shift 127: ties between walk indices 3, 67 and 130, between 64 and 65, and index 254 one record ahead
    of index 0 — candidates that pick_mode meets in different lanes and in different trips of its loop — a different
    pattern on each axis of a frame; applied (min_share_q8 0) and with a share just missed.  Hand values."""
    seen = 0
    for (thr, margin, ms, q8), names, mv, off, sd, want_c, want_i, plain in gi.lane_batches():
        s = gpu_scanner_factory(gi.hand_params(thr, margin))
        for label, fl, ce, info in gmc_both_layouts(s, mv, off, sd, ms, q8, "/".join(names)):
            assert_counts_equal(ce, want_c, label, got_f=fl, want_f=(want_c >= 1).astype(np.uint8))
            assert_info_equal(info, want_i, label)
        hf, hc, hi = s.scan_gmc(m.FrameBatch(mv, off, None, sd), ms, q8)
        assert_counts_equal(hc, want_c, "host entry " + "/".join(names), got_f=hf, want_f=(want_c >= 1).astype(np.uint8))
        assert_info_equal(hi, want_i, "host entry " + "/".join(names))
        seen += len(names)
    assert seen == len(gi.LANES) == 7


# ------------------------------------------------------------------ 9. has_sd == NULL

def test_has_sd_null_scans_every_frame_that_owns_records(gpu_scanner_factory):
    """include/mtgpu_gmc.h: "has_sd == NULL: the frame owns no record".  The hand batches without has_sd on both entry
    points: the hand cases as before, the pans of 9 behind them by gi.follower_by_hand, the empty frame 0 everywhere."""
    for batches in (gi.hand_batches(), gi.lane_batches()):
        for (thr, margin, ms, q8), names, mv, off, sd, want_c, want_i, plain in batches:
            fc, fi = gi.follower_by_hand(margin, ms)
            want_c, want_i = want_c.copy(), want_i.copy()
            want_c[1::2], want_i[1::2] = fc, fi
            want_f = (want_c >= 1).astype(np.uint8)
            s = gpu_scanner_factory(gi.hand_params(thr, margin))
            for label, fl, ce, info in gmc_both_layouts(s, mv, off, None, ms, q8, "no has_sd " + "/".join(names)):
                assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
                assert_info_equal(info, want_i, label)
            hf, hc, hi = s.scan_gmc(m.FrameBatch(mv, off, None, None), ms, q8)
            assert_counts_equal(hc, want_c, "host entry, no has_sd " + "/".join(names), got_f=hf, want_f=want_f)
            assert_info_equal(hi, want_i, "host entry, no has_sd " + "/".join(names))
            if "no_records" in names:
                f = 2 * names.index("no_records")
                assert int(off[f]) == int(off[f + 1]) and not gi.info_rows(hi)[f].any() and hc[f] == 0 and hf[f] == 0


# ------------------------------------------------------------------ 10. the host entry on a batch that starts at record 4097

def test_host_entry_rebases_the_records(gpu_scanner_factory):
    """mtgpu_scan_frames_gmc copies only the records frame_off spans and plans with rebase = frame_off[0]: pan_batch()
    inside a larger array, frame_off[0] == 4097 and 1000 records behind frame_off[-1], equals the call on the batch alone
    and the model."""
    mv, off, sd, _, _ = gi.pan_batch()
    big, off2 = gi.embedded_pan_batch()
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1)
    s = gpu_scanner_factory(p)
    want_f, want_c, want_i = gm.gmc_batch(p, mv, off, sd, gi.PAN_MAX_SHIFT, 128)
    af, ac, ai = s.scan_gmc(m.FrameBatch(mv, off, None, sd), gi.PAN_MAX_SHIFT, 128)
    gf, gc, gi_ = s.scan_gmc(m.FrameBatch(big, off2, None, sd), gi.PAN_MAX_SHIFT, 128)
    assert_counts_equal(gc, want_c, "embedded batch against the model", got_f=gf, want_f=want_f)
    assert_info_equal(gi_, gi.info_rows(want_i), "embedded batch against the model")
    assert_counts_equal(gc, ac, "embedded batch against the aligned call", got_f=gf, want_f=af)
    assert gi_.tobytes() == ai.tobytes()
    # and without has_sd: the same frames own the same records
    nf, nc, ni = s.scan_gmc(m.FrameBatch(big, off2, None, None), gi.PAN_MAX_SHIFT, 128)
    wf, wc, wi = gm.gmc_batch(p, mv, off, None, gi.PAN_MAX_SHIFT, 128)
    assert_counts_equal(nc, wc, "embedded batch without has_sd", got_f=nf, want_f=wf)
    assert_info_equal(ni, gi.info_rows(wi), "embedded batch without has_sd")


# ------------------------------------------------------------------ 11. 2^24 records in one frame

def test_support_and_pick_in_64_bits_on_2_pow_24_records(gpu_scanner_factory):
    """gi.HUGE: n_x * 256 = 2^32 + 256 against 256 * n_in = 2^32 + 512 — unsupported, centres 2 — and against 255 * n_in —
    supported, centres 0.  Compact records, repeated on the device from two 8-byte patterns (134 MB; the host never
    holds them); one workgroup streams the frame twice."""
    import time
    import torch
    a, b, c = m.pack_records(dei.voters(gi.HUGE_TRIPLE, 4)).view(np.int64).tolist()
    d_rec = torch.empty(gi.HUGE_N, dtype=torch.int64, device="cuda")
    d_rec[0::2], d_rec[1::2] = a, b
    d_rec[-1] = c
    d_off = torch.tensor([0, gi.HUGE_N], dtype=torch.int64, device="cuda")
    d_sd = torch.ones(1, dtype=torch.uint8, device="cuda")
    s = gpu_scanner_factory(gi.hand_params(16.0, 0))
    for q8, (want_i, want_c) in gi.HUGE.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, 16, q8, True)
        print(f"2^24 + 2 records, min_share_q8 {q8}: {1e3 * (time.perf_counter() - t0):.1f} ms for the call")
        assert_info_equal(info, [want_i], f"2^24 + 2 records, min_share_q8 {q8}")
        assert_counts_equal(ce, [want_c], f"2^24 + 2 records, min_share_q8 {q8}", got_f=fl, want_f=[int(want_c >= 1)])


# ------------------------------------------------------------------ 12. more frames than one trip of the clear kernels

@pytest.mark.parametrize("which", ["gmc", "zones", "blobs"])
def test_clear_kernels_second_trip(gpu_scanner_factory, which):
    """gi.clear_batch(): 262 144 + 300 frames, so that gmc_clear_kernel (1024 x 256 lanes) writes the elements from
    262 144 on in a second trip of its loop; all of them read 0 only because of it, but the four planted frames (0, the
    last of the first trip, the first of the second, the last), which read the hand values.  gmc: all three outputs,
    then centres alone.  zones, blobs: the same batch through the masked scan (one stream, every cell kept) and the
    blobs, whose clear kernels have the same loop, against the plain scan's hand values of those frames."""
    import torch
    from test_gpu_blobs import JUNK_BOX, device_blobs
    from test_gpu_zones import device_zones, keep_tensor, soff_tensor
    mv, off, sd, planted = gi.clear_batch()
    F, idx = gi.CLEAR_FRAMES, list(planted)
    thr, margin, _, ms, q8, info1, c1, plain1 = gi.HAND[gi.CLEAR_CASE]
    s = gpu_scanner_factory(gi.hand_params(thr, margin))
    want_c, want_i, want_p = np.zeros(F, dtype=np.uint32), np.zeros((F, 7), dtype=np.int64), np.zeros(F, dtype=np.uint32)
    want_c[idx], want_i[idx], want_p[idx] = c1, info1, plain1
    want_box = np.full((F, 4), 0xFFFF, dtype=np.int64)
    want_box[idx] = gi.CLEAR_BOX
    assert JUNK_BOX != 0xFFFF
    for compact in (False, True):
        label = f"{F} frames, {'compact' if compact else '40-byte'}"
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        if which == "gmc":
            fl, ce, info = device_gmc(s, d_rec, d_off, d_sd, ms, q8, compact)
            assert_counts_equal(ce, want_c, label, got_f=fl, want_f=(want_c >= 1).astype(np.uint8))
            assert_info_equal(info, want_i, label)
            alone = torch.full((F,), JUNK, dtype=torch.int32, device="cuda")
            s.scan_gmc_device(d_rec, d_off, d_sd, ms, q8, compact=compact, flags=False, centres=alone, info=False)
            torch.cuda.synchronize()
            assert_counts_equal(alone.cpu().numpy().view(np.uint32), want_c, label + ", centres alone")
        elif which == "zones":
            d_soff, d_keep = soff_tensor([0, F]), keep_tensor(np.ones((1, gi.GH, gi.GW), dtype=bool))
            zf, zc, za = device_zones(s, d_rec, d_off, d_sd, d_soff, d_keep, compact)
            assert_counts_equal(zc, want_p, label + ", masked scan", got_f=zf, want_f=(want_p >= 1).astype(np.uint8))
            assert_counts_equal(za, want_p, label + ", masked scan centres_all")
        else:
            got = device_blobs(s, d_rec, d_off, d_sd, compact)
            for k, w in (("centres", want_p), ("blobs", want_p > 0), ("largest", want_p)):
                assert_counts_equal(got[k], w, f"{label}, blobs: {k}")
            assert np.array_equal(got["flags"], (want_p >= 1).astype(np.uint8)), label + ", blobs: flags"
            bad = np.flatnonzero((got["box"].astype(np.int64).reshape(-1, 4) != want_box).any(axis=1))
            assert bad.size == 0, (label, "blobs: boxes differ at", bad[:8].tolist(), got["box"].reshape(-1, 4)[bad[:4]].tolist())
