"""GPU tier: object tracks (include/mtgpu_tracks.h) against the sequential model of tests/tracks_model.py and the hand
values of tests/tracks_inputs.py.  Every comparison is exact.  The lists are built in numpy; the shapes are the smallest
at which a carry between the lanes of a group, between groups, waves or tiles, a stream boundary or a clamp can go wrong
(T = frames_per_tile, sixteen lanes a frame, sixteen frames a group)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, mvfile, objects, tracks

import objects_model as om
import persist_inputs as pi
import tracks_inputs as ti
import tracks_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = tracks.OUTPUTS
VIEW = {"pred": np.uint8, "flags": np.uint8}


@pytest.fixture(scope="module")
def scanner(gpu_scanner_factory):
    return gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))


@pytest.fixture(scope="module")
def T():
    return tracks.preview(16)["frames_per_tile"]


def model(c, **kw):
    a = ti.settings(c)
    a.update(kw)
    return tm.tracks(c["flags"], c["lists"], c["soff"], c["sd"], **a)


def on_device(c):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    n, k = c["lists"].shape
    return (t(c["flags"]), t(c["lists"].view(np.int32).reshape(n, k, 4)), t(c["soff"].view(np.int64)), None if c["sd"] is None else t(c["sd"]))


def run_device(s, c, want=ALL, out=None, **kw):
    import torch
    a = ti.settings(c)
    a.update(kw)
    d_flags, d_list, d_soff, d_sd = on_device(c)
    res = tracks.link_device(s, d_flags, d_list, d_soff, d_sd, want=want, out=out, **a)
    torch.cuda.synchronize()
    return {o: (None if v is None else v.cpu().numpy().view(VIEW.get(o, np.uint32))) for o, v in res.items()}


def assert_case(s, c, label, wants=(ALL,), want=None, **kw):
    want = model(c, **kw) if want is None else want
    for w in wants:
        got = run_device(s, c, w, **kw)
        for o in ALL:
            if o in w:
                bad = np.argwhere(got[o] != want[o])
                assert not len(bad), (label, w, o, bad[:6].tolist(), got[o][got[o] != want[o]][:6].tolist(), want[o][got[o] != want[o]][:6].tolist())
            else:
                assert got[o] is None
    return want


# ------------------------------------------------------------------ 1. the hand cases

@pytest.mark.parametrize("k", ti.HAND_K)
def test_hand_cases(scanner, k):
    """Every hand case at k = 1, 2, 15 (an idle lane in every group) and 16: device call, host call, and embedded as one
    stream of four (consequence D: the ids move by the stream's first frame times k)."""
    for name in ti.HAND:
        c, hand = ti.hand_case(name, k)
        assert_case(scanner, c, name, want=hand)
        got = tracks.link(scanner, c["flags"], c["lists"], c["soff"], c["sd"], **ti.settings(c))
        assert all(np.array_equal(got[o], hand[o]) for o in ALL), name
        e, sl, moved = ti.embed(c, hand, k)
        want = assert_case(scanner, e, name + " embedded")
        assert all(np.array_equal(want[o][sl], moved[o]) for o in ALL), name


# ------------------------------------------------------------------ 2. tile seams

@pytest.mark.parametrize("k", (1, 2, 16))
def test_tile_seams(scanner, T, k):
    cases = ti.seam_cases(T, k)
    assert len(cases) == 8 + 2 + 4
    for name, c in cases.items():
        want = assert_case(scanner, c, f"{name} k={k}")
        if name.startswith("steady"):                       # one track through every seam
            assert want["track"].tolist() == [len(c["flags"])] * len(c["flags"])
        if name == "tile of quiet":
            assert want["track"][[3, 4, T + 40, T + 41]].tolist() == [4] * 4
        if name == "tile of quiet, bounded":
            assert want["track"][[3, 4, T + 40, T + 41]].tolist() == [2] * 4
        if name.startswith("split@") and k > 1:
            f = int(name.split("@")[1])
            assert want["pred"][f, :2].tolist() == [0, 0] and want["age"][f, :2].tolist() == [f + 1, f + 1]


# ------------------------------------------------------------------ 3. streams

def test_seventy_streams_and_frames_outside_them(scanner, T):
    import torch
    c, lens = ti.streams_case(T, 3)
    assert len(lens) == 70 and lens[:8] == [0, 1, 2, 16, T + 1, 0, 0, 1]
    want = assert_case(scanner, c, "70 streams")
    n, k = c["lists"].shape
    outside = np.r_[0:3, n - 5:n]
    assert (c["flags"][outside] != 0).all() and (want["id"][outside] == ti.NO_ID).all() and not want["track"][outside].any()
    # the frames outside are written, not left alone: the outputs start out as junk
    dev = torch.device("cuda", 0)
    out = {o: torch.full((n, k) if o in ("pred", "age", "id", "len") else (n,), 7, dtype=torch.uint8 if o in VIEW else torch.int32, device=dev)
           for o in ALL}
    got = run_device(scanner, c, out=out)
    assert all(np.array_equal(got[o], want[o]) for o in ALL)
    # offsets past n_frames are read as n_frames (the device entry point trusts them, the kernels clamp them)
    far = dict(c, soff=c["soff"].copy())
    far["soff"][-1] = n + 1000
    far["soff"][-2] = n + 7
    clamped = dict(c, soff=np.minimum(far["soff"], n))
    assert_case(scanner, far, "offsets past the end", want=model(clamped))


# ------------------------------------------------------------------ 4. random soak

@pytest.mark.parametrize("chunk", range(2))
def test_random_soak(scanner, T, chunk):
    for seed in range(chunk * 8, chunk * 8 + 8):
        c = ti.random_case(600 + seed, max_streams=5, max_len=T + 150)
        assert_case(scanner, c, f"draw {seed}")


# ------------------------------------------------------------------ 5. consequence A against persistence, on the same buffers

def test_k1_is_persistence(scanner, T):
    import torch
    for seed in range(6):
        pc = pi.random_case(900 + seed, max_streams=5, max_len=T + 120, with_box=bool(seed & 1), with_sd=bool(seed & 2))
        c, box = ti.persist_twin(pc)
        d_flags, d_list, d_soff, d_sd = on_device(c)
        d_box = d_list[:, 0, 2:].contiguous().view(torch.int16)           # the entry's bounds
        assert np.array_equal(d_box.cpu().numpy().view(np.uint16), box.view(np.uint16).reshape(-1, 4))
        got = tracks.link_device(scanner, d_flags, d_list, d_soff, d_sd, 1, c["max_dropout"], c["reach"], c["min_track"])
        per = scanner.persist_device(d_flags, d_soff, d_sd, d_box, c["min_track"], c["max_dropout"], c["reach"])
        torch.cuda.synchronize()
        assert torch.equal(got["age"][:, 0], per["pos"]) and torch.equal(got["len"][:, 0], per["run"]), seed
        assert torch.equal(got["track"], per["run"]) and torch.equal(got["flags"], per["flags"]), seed
        assert int(per["run"].max().item()) > 1


# ------------------------------------------------------------------ 6. consequence C

def test_track_feeds_the_unchanged_sweep(scanner):
    import torch
    c, pts = ti.sweep_case()
    dev = torch.device("cuda", 0)
    d_flags, d_list, d_soff, d_sd = on_device(c)
    d_pts = torch.from_numpy(pts).to(dev)
    S = len(c["soff"]) - 1
    mp = m.MergeParams(duration=40.0, max_gap_sec=1.0, padding_sec=0.5, min_savings_pct=5.0)
    d_mp = torch.from_numpy(np.tile(mp.to_record().view(np.uint8), S).copy()).to(dev)
    levels = [1, 2, 3, 5]
    a = (c["min_cells"], c["max_dropout"], c["reach"])
    res = tracks.link_device(scanner, d_flags, d_list, d_soff, d_sd, *a, 1, want=("track",))
    seg, r8 = scanner.sweep_streams_device(res["track"], d_pts, d_soff, d_mp, levels, seg_cap=64)
    kept = []
    for i, lv in enumerate(levels):
        fo = tracks.link_device(scanner, d_flags, d_list, d_soff, d_sd, *a, lv, want=("flags",))["flags"]
        mseg, mres = scanner.merge_streams_device(fo, d_pts, d_soff, d_mp, seg_cap=64)
        torch.cuda.synchronize()
        assert seg[i].cpu().numpy().tobytes() == mseg.cpu().numpy().tobytes(), lv
        assert r8[i].cpu().numpy().tobytes() == mres.cpu().numpy().tobytes(), lv
        assert np.array_equal(fo.cpu().numpy(), model(c, min_track=lv)["flags"])
        kept.append(int(fo.sum().item()))
    assert kept[0] > kept[1] > kept[2] > kept[3] > 0            # every level bites


# ------------------------------------------------------------------ 7. end to end: object scan into tracks on the device

def test_end_to_end_two_movers_and_a_flicker(gpu_scanner_factory):
    import torch
    p, mv, off, sd = ti.e2e_batch()
    k = 4
    lists = om.model_batch(p, mv, off, sd, k, 1)
    flags = om.flags_np(p, lists["centres"], lists["objects"], 1)
    soff = np.array([0, len(flags)], dtype=np.uint64)
    want = tm.tracks(flags, lists["list"], soff, sd, reach=1, min_track=2)
    # what the picture says: the 3 x 3 mover lives 21 motion frames (frame 12 is a key frame), the 2 x 2 mover 11, the flicker 1
    assert want["len"][ti.E2E_FLICKER].tolist() == [21, 11, 1, 0] and want["id"][ti.E2E_FLICKER].tolist() == [2 * k, 6 * k + 1, 9 * k + 2, ti.NO_ID]
    assert int((want["age"] == 1).sum()) == 3 and want["track"][[0, 1, 12]].tolist() == [0, 0, 0]
    s = gpu_scanner_factory(p)
    dev = torch.device("cuda", 0)
    d_rec = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_sd = torch.from_numpy(sd.copy()).to(dev)
    d_soff = torch.from_numpy(soff.view(np.int64).copy()).to(dev)
    scan = objects.scan_device(s, d_rec, d_off, d_sd, k, 1, 1, want=("flags", "list"))
    got = tracks.link_device(s, scan["flags"], scan["list"], d_soff, d_sd, 1, 0, 1, 2)
    torch.cuda.synchronize()
    assert np.array_equal(scan["flags"].cpu().numpy(), flags)
    for o in ALL:
        assert np.array_equal(got[o].cpu().numpy().view(VIEW.get(o, np.uint32)), want[o]), o


# ------------------------------------------------------------------ 8. each output alone

def test_each_output_alone(scanner, T):
    """One output non-NULL at a time: len, track and flags_out alone keep the ids in the workspace; pred, age and id alone
    launch no finish kernel."""
    c = ti.random_case(77, k=5, max_streams=3, max_len=T + 40)
    assert_case(scanner, c, "alone", wants=tuple((o,) for o in ALL) + (("len", "flags"), ("pred", "track")))
    before = scanner.stats()["pool_reserved_bytes"]
    run_device(scanner, c)
    assert scanner.stats()["pool_reserved_bytes"] == before           # nothing comes from the scratch ring
    import torch
    d_flags, d_list, d_soff, d_sd = on_device(c)
    with pytest.raises(m.MtgpuError) as ei:
        tracks.link_device(scanner, d_flags, d_list, d_soff, d_sd, want=("flags",), out={"flags": d_flags})
    assert ei.value.code == _abi.MT_ERR_INVALID and "d_flags_out overlaps d_flags" in str(ei.value)
    with pytest.raises(m.MtgpuError) as ei:
        tracks.link_device(scanner, d_flags, d_list, d_soff, d_sd, reach=65536)
    assert ei.value.code == _abi.MT_ERR_INVALID and "reach" in str(ei.value)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 9. contract, example, command

def _build_c(tmp_path, src, name, hip=False):
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / name)
    extra = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + pkg,
                           "-lmtgpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"] + extra)
    return exe


def test_every_refusal_and_every_buffer(tmp_path):
    """tests/c/abi_tracks_canaries.c: each MT_ERR_INVALID with the argument named and the outputs untouched, buffers at
    exactly their stated sizes with canaries behind them."""
    exe = _build_c(tmp_path, os.path.join(ROOT, "tests", "c", "abi_tracks_canaries.c"), "abi_tracks_canaries", hip=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all tracks buffers respected" in out.stdout


def test_plain_c_tracks_example(tmp_path):
    """examples/tracks_example.c prints the tracks the model gives for its lists: two movers and one flicker."""
    exe = _build_c(tmp_path, os.path.join(ROOT, "examples", "tracks_example.c"), "tracks_example")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in ("3 tracks", "track 0: 6 frames", "track 9: 8 frames", "track 44: 1 frames", "MIN_TRACK 1: 11 motion frames",
                 "MIN_TRACK 2: 10 motion frames", "MIN_TRACK 7: 8 motion frames", "MIN_TRACK 9: 0 motion frames"):
        assert line in out.stdout, out.stdout


def test_end_to_end_command(tmp_path, capsys):
    """A .mtmv of the end-to-end batch, then `python -m mvtrim_amd.tracks --json` in a fresh child process and the table
    in this one."""
    p, mv, off, sd = ti.e2e_batch()
    n = len(sd)
    frames = [mv[int(off[f]):int(off[f + 1])] if sd[f] else None for f in range(n)]
    path = str(tmp_path / "e2e.mtmv")
    mvfile.write_mtmv(path, 16 * ti.E2E_GRID[0], 16 * ti.E2E_GRID[1], 1, 90000, 30.0, n / 30.0, [3000 * f for f in range(n)], frames)
    common = [path, "--vectors-needed", "1", "--vertical-mask", "0", "--max-gap-sec", "0.5", "--padding-sec", "0.1", "--top", "4"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.tracks"] + common + ["--min-track", "2,12", "--json"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    doc = json.loads(out.stdout)
    rows = {r["min_track"]: r for r in doc["levels"]}
    assert sorted(rows) == [1, 2, 12] and doc["top"] == 4 and doc["reach"] == 1
    assert rows[1]["motion_frames"] == rows[2]["motion_frames"] == rows[12]["motion_frames"] == 21        # the long mover is in every motion frame
    assert doc["tracks"] == 3 and doc["longest_track"] == 21
    assert doc["track_lengths"]["1"] == 1 and doc["track_lengths"]["10-29"] == 2
    assert tracks.main(common + ["--min-track", "22"]) == 0
    text = capsys.readouterr().out
    assert "3 tracks" in text and "the longest is 21 motion frames deep" in text
    table = [ln.split() for ln in text.splitlines() if ln[:1].isdigit()]
    assert [int(r[0]) for r in table] == [1, 22] and [int(r[1]) for r in table] == [21, 0]
    assert "track lengths: 1: 1" in text
