"""GPU tier: temporal persistence (include/mtgpu_persist.h) against the sequential model of tests/persist_model.py.  Every
comparison is exact.  All three outputs are requested together and each one alone; the shapes are the smallest at which a
carry between lanes, waves or tiles, a stream boundary or a clamp can go wrong (T = frames_per_tile, W = 64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, mvfile, persist

import blobs_model as bm
import persist_inputs as pi
import persist_model as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTS = (("flags", "run", "pos"), ("flags",), ("run",), ("pos",))


@pytest.fixture(scope="module")
def scanner(gpu_scanner_factory):
    return gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))


@pytest.fixture(scope="module")
def plan():
    return m.persist_preview()


def model(c, **kw):
    a = dict(min_run=c["min_run"], max_dropout=c["max_dropout"], reach=c["reach"])
    a.update(kw)
    return pm.persist(c["flags"], c["soff"], c["sd"], c["box"], **a)


def on_device(c):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    return (t(c["flags"]), t(c["soff"].view(np.int64)), None if c["sd"] is None else t(c["sd"]),
            None if c["box"] is None else t(c["box"].view(np.int16).reshape(-1, 4)))


def run_device(s, c, want=WANTS[0], **kw):
    import torch
    a = dict(min_run=c["min_run"], max_dropout=c["max_dropout"], reach=c["reach"])
    a.update(kw)
    d_flags, d_soff, d_sd, d_box = on_device(c)
    res = s.persist_device(d_flags, d_soff, d_sd, d_box, want=want, **a)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy().view(np.uint8 if k == "flags" else np.uint32)) for k, v in res.items()}


def assert_case(s, c, label, wants=WANTS, want=None, **kw):
    want = model(c, **kw) if want is None else want
    for w in wants:
        got = run_device(s, c, w, **kw)
        for k in ("flags", "run", "pos"):
            if k in w:
                bad = np.flatnonzero(got[k] != want[k])
                assert not len(bad), (label, w, k, bad[:8].tolist(), got[k][bad[:8]].tolist(), want[k][bad[:8]].tolist())
            else:
                assert got[k] is None
    return want


# ------------------------------------------------------------------ 1. the worked cases

@pytest.mark.parametrize("name", list(pi.WORKED))
def test_worked_cases(scanner, name):
    c, run, pos, flags_out = pi.WORKED[name]
    hand = {"flags": np.array(flags_out, dtype=np.uint8), "run": np.array(run, dtype=np.uint32), "pos": np.array(pos, dtype=np.uint32)}
    assert_case(scanner, c, name, want=hand)
    # the host entry point
    got = scanner.persist(c["flags"], c["soff"], c["sd"], c["box"], c["min_run"], c["max_dropout"], c["reach"])
    assert all(np.array_equal(got[k], hand[k]) for k in hand), name
    # as stream 3 of 5 (G)
    e, sl = pi.embed(c)
    want = assert_case(scanner, e, name + " embedded")
    assert all(np.array_equal(want[k][sl], hand[k]) for k in hand)


# ------------------------------------------------------------------ 2. seams

def test_seams(scanner, plan):
    T, wg = plan["frames_per_tile"], plan["workgroup"]
    cases = pi.seam_cases(T, wg)
    assert len(cases) == 8 * (2 + 6 + 4) + 4
    for name, c in cases.items():
        assert_case(scanner, c, name, wants=WANTS[:1])
    # each output alone on the cases that cross a tile
    for name in (f"start@{T}", f"end@{T}", f"streak6/5@{T}", f"tile-back-T-linked@{T - 1}", f"tile-back-Q-apart@{2 * T}", "all-M", "whole-stream-run"):
        assert_case(scanner, cases[name], name, wants=WANTS[1:])


# ------------------------------------------------------------------ 3. stream shapes

def test_stream_shapes_and_frames_outside_the_streams(scanner, plan):
    import torch
    c = pi.shapes_case(plan["frames_per_tile"])
    want = assert_case(scanner, c, "shapes")
    # the frames outside are written, not left alone: the outputs start out non-zero
    d_flags, d_soff, d_sd, d_box = on_device(c)
    n = len(c["flags"])
    out = {"flags": torch.full((n,), 7, dtype=torch.uint8, device=d_flags.device),
           "run": torch.full((n,), 7, dtype=torch.int32, device=d_flags.device),
           "pos": torch.full((n,), 7, dtype=torch.int32, device=d_flags.device)}
    res = scanner.persist_device(d_flags, d_soff, d_sd, d_box, c["min_run"], c["max_dropout"], c["reach"], out=out)
    torch.cuda.synchronize()
    for k in out:
        assert res[k] is out[k] and np.array_equal(out[k].cpu().numpy().astype(np.int64), want[k].astype(np.int64)), k
    outside = np.r_[0:3, n - 5:n]
    assert not any(want[k][outside].any() for k in want)
    # offsets past n_frames are read as n_frames (the device entry point trusts them, the kernel clamps them)
    far = dict(c)
    far["soff"] = c["soff"].copy()
    far["soff"][-1] = n + 1000
    clamped = dict(c)
    clamped["soff"] = c["soff"].copy()
    clamped["soff"][-1] = n
    assert_case(scanner, far, "offset past the end", wants=WANTS[:1], want=model(clamped))


# ------------------------------------------------------------------ 4. parameters

def test_parameters(scanner):
    c = pi.random_case(7, max_streams=3, max_len=700, with_box=True, with_sd=True)
    assert {2, 255} <= set(c["flags"].tolist())
    is_m = (c["flags"] != 0).astype(np.uint8)
    for mr in (0, 1, 2, 0xFFFFFFFF):
        want = assert_case(scanner, c, f"min_run {mr}", wants=(("flags",),), min_run=mr)
        assert set(want["flags"].tolist()) <= {0, 1}
        if mr <= 1:
            assert np.array_equal(want["flags"], is_m)                                   # A
        if mr == 0xFFFFFFFF:
            assert not want["flags"].any()
    for md in (0, 0xFFFFFFFF):
        assert_case(scanner, c, f"max_dropout {md}", wants=WANTS[:1], max_dropout=md)
    for reach in (0, 65535):
        assert_case(scanner, c, f"reach {reach}", wants=WANTS[:1], reach=reach)
    # B: no boxes, no dropout limit — every M frame reads its stream's M count
    nb = dict(c, box=None)
    got = assert_case(scanner, nb, "B", wants=WANTS[:1], max_dropout=0xFFFFFFFF)
    for s in range(len(c["soff"]) - 1):
        sl = slice(int(c["soff"][s]), int(c["soff"][s + 1]))
        assert np.array_equal(got["run"][sl], np.where(is_m[sl] != 0, int(is_m[sl].sum()), 0))
    # C: neither boxes nor has_sd — blocks of consecutive flags; and has_sd given changes the answer
    plain = dict(c, box=None, sd=None)
    got_plain = assert_case(scanner, plain, "C", wants=WANTS[:1], max_dropout=0)
    got_sd = assert_case(scanner, nb, "C with has_sd", wants=WANTS[:1], max_dropout=0)
    assert (got_sd["run"] >= got_plain["run"]).all() and (got_sd["run"] > got_plain["run"]).any()
    # reach is ignored without boxes
    assert np.array_equal(run_device(scanner, nb, reach=0)["run"], run_device(scanner, nb, reach=65535)["run"])


# ------------------------------------------------------------------ 5. random soak

def test_random_soak(scanner, plan):
    T = plan["frames_per_tile"]
    for seed in range(40):
        c = pi.random_case(500 + seed, max_streams=12, max_len=2 * T + 300, with_box=bool(seed & 1), with_sd=bool(seed & 2))
        assert_case(scanner, c, f"draw {seed}", wants=WANTS[:1] if seed % 4 else WANTS)


def test_one_long_stream(scanner):
    fl, sd, bx = pi.long_stream(300000)
    c = pi.case(fl, None, sd, bx, min_run=5, max_dropout=2, reach=4)
    want = assert_case(scanner, c, "300000 frames", wants=WANTS[:1])
    assert int(want["run"].max()) > 30 and int((want["pos"] == 1).sum()) > 1000


# ------------------------------------------------------------------ 6. consequence E

def test_run_feeds_the_unchanged_sweep(scanner):
    import torch
    c, pts = pi.sweep_case()
    dev = torch.device("cuda", 0)
    d_flags, d_soff, d_sd, _ = on_device(c)
    d_pts = torch.from_numpy(pts).to(dev)
    S = len(c["soff"]) - 1
    mp = m.MergeParams(duration=40.0, max_gap_sec=1.0, padding_sec=0.5, min_savings_pct=5.0)
    d_mp = torch.from_numpy(np.tile(mp.to_record().view(np.uint8), S).copy()).to(dev)
    levels = [1, 2, 3, 5]
    res = scanner.persist_device(d_flags, d_soff, d_sd, None, 1, c["max_dropout"], 0, want=("run",))
    seg, r8 = scanner.sweep_streams_device(res["run"], d_pts, d_soff, d_mp, levels, seg_cap=64)
    kept = []
    for i, lv in enumerate(levels):
        fo = scanner.persist_device(d_flags, d_soff, d_sd, None, lv, c["max_dropout"], 0, want=("flags",))["flags"]
        mseg, mres = scanner.merge_streams_device(fo, d_pts, d_soff, d_mp, seg_cap=64)
        torch.cuda.synchronize()
        assert seg[i].cpu().numpy().tobytes() == mseg.cpu().numpy().tobytes(), lv
        assert r8[i].cpu().numpy().tobytes() == mres.cpu().numpy().tobytes(), lv
        assert np.array_equal(fo.cpu().numpy(), model(c, min_run=lv)["flags"])
        kept.append(int(fo.sum().item()))
    assert kept[0] > kept[1] > kept[2] > kept[3] > 0            # every level bites


# ------------------------------------------------------------------ 7. end to end on synth

def test_end_to_end_flashes_against_one_event(gpu_scanner_factory):
    p, mv, off, sd = pi.e2e_stream()
    # what the model expects, CPU only: the blob model's flags and boxes, then the persistence model
    stats = bm.model_batch(p, mv, off, sd)
    flags = bm.flags_np(p, stats["centres"], stats["largest"], 1)
    assert np.flatnonzero(flags).tolist() == sorted(list(pi.E2E_FLASHES) + pi.E2E_KEPT)
    soff = np.array([0, len(flags)], dtype=np.uint64)
    want = pm.persist(flags, soff, sd, stats["box"], min_run=3, max_dropout=0, reach=1)
    assert np.flatnonzero(want["flags"]).tolist() == pi.E2E_KEPT == list(range(121, 150))
    assert all(want["run"][f] == 1 for f in pi.E2E_FLASHES) and (want["run"][pi.E2E_KEPT] == 29).all()
    # without the boxes the flash in front of the event's key frame joins the event
    loose = pm.persist(flags, soff, sd, None, min_run=3)
    assert np.flatnonzero(loose["flags"]).tolist() == [119] + pi.E2E_KEPT

    s = gpu_scanner_factory(p)
    got = s.scan_blobs(m.FrameBatch(mv, off, None, sd), 1)
    assert np.array_equal(got["flags"], flags) and np.array_equal(got["box"].view(np.uint16).reshape(-1, 4), stats["box"])
    res = s.persist(got["flags"], soff, sd, got["box"], min_run=3, max_dropout=0, reach=1)
    assert all(np.array_equal(res[k], want[k]) for k in want)
    assert np.flatnonzero(res["flags"]).tolist() == pi.E2E_KEPT
    res = s.persist(got["flags"], soff, sd, None, min_run=3)
    assert np.flatnonzero(res["flags"]).tolist() == [119] + pi.E2E_KEPT


# ------------------------------------------------------------------ 8. contract, example, command

def _build_c(tmp_path, src, name, hip=False):
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / name)
    extra = ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-L/opt/rocm/lib", "-lamdhip64"] if hip else []
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + pkg,
                           "-lmtgpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"] + extra)
    return exe


def test_every_refusal_and_every_buffer(tmp_path):
    """tests/c/abi_persist_canaries.c: each MT_ERR_INVALID with the argument named and the outputs untouched, buffers at
    exactly their stated sizes with canaries behind them, pool_reserved_bytes unchanged."""
    exe = _build_c(tmp_path, os.path.join(ROOT, "tests", "c", "abi_persist_canaries.c"), "abi_persist_canaries", hip=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all persistence buffers respected" in out.stdout


def test_a_call_takes_nothing_from_the_scratch_ring(scanner):
    c = pi.random_case(3, with_box=True, with_sd=True)
    before = scanner.stats()["pool_reserved_bytes"]
    run_device(scanner, c)
    assert scanner.stats()["pool_reserved_bytes"] == before
    # refusals through the Python layer name the argument
    import torch
    d_flags, d_soff, d_sd, d_box = on_device(c)
    with pytest.raises(m.MtgpuError) as ei:
        scanner.persist_device(d_flags, d_soff, d_sd, d_box, want=("flags",), out={"flags": d_flags})
    assert ei.value.code == _abi.MT_ERR_INVALID and "d_flags_out overlaps d_flags" in str(ei.value)
    with pytest.raises(m.MtgpuError) as ei:
        scanner.persist_device(d_flags, d_soff, d_sd, d_box, reach=65536)
    assert ei.value.code == _abi.MT_ERR_INVALID and "reach" in str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(d_flags.cpu().numpy(), c["flags"])


def test_plain_c_persist_example(tmp_path):
    """examples/persist_example.c prints the counts the model gives for its stream."""
    fl, sd = pi.example_flags()
    lines = []
    for mr in (1, 3):
        got = pm.persist(fl, [0, len(fl)], sd, None, min_run=mr)
        ts = np.flatnonzero(got["flags"]) / 10.0
        segments = 1 + int((np.diff(ts) > 1.0).sum())          # MAX_GAP_SEC 1: a gap strictly greater splits
        lines.append(f"MIN_RUN {mr}: {int(got['flags'].sum())} motion frames in {segments} segments")
    assert lines == ["MIN_RUN 1: 36 motion frames in 8 segments", "MIN_RUN 3: 29 motion frames in 1 segments"]
    exe = _build_c(tmp_path, os.path.join(ROOT, "examples", "persist_example.c"), "persist_example")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    for line in lines + ["longest run: 29 frames"]:
        assert line in out.stdout, out.stdout


def test_end_to_end_command(gpu_scanner_factory, tmp_path, capsys):
    """A .mtmv of the end-to-end stream, then `python -m mvtrim_amd.persist --blobs --json` in a fresh child process and the
    centre-scan table in this one."""
    p, mv, off, sd = pi.e2e_stream()
    frames = [mv[int(off[f]):int(off[f + 1])] if sd[f] else None for f in range(len(sd))]
    path = str(tmp_path / "e2e.mtmv")
    mvfile.write_mtmv(path, 1920, 1080, 1, 90000, 30.0, len(sd) / 30.0, [3000 * f for f in range(len(sd))], frames)
    common = [path, "--vectors-needed", "1", "--clusters-needed", "1", "--max-gap-sec", "0.5", "--padding-sec", "0.1"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.persist"] + common + ["--blobs", "--min-run", "3", "--json"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    doc = json.loads(out.stdout)
    rows = {r["min_run"]: r for r in doc["levels"]}
    assert sorted(rows) == [1, 3] and doc["blobs"] and doc["reach"] == 1
    assert rows[1]["motion_frames"] == len(pi.E2E_KEPT) + len(pi.E2E_FLASHES) and rows[1]["segments"] == 4       # 119 merges with the event
    assert rows[3]["motion_frames"] == rows[3]["frames_kept"] == len(pi.E2E_KEPT) and rows[3]["segments"] == 1
    assert doc["runs"] == 5 and doc["longest_run"] == 29 and doc["run_lengths"]["1"] == 4 and doc["run_lengths"]["10-29"] == 1
    assert 0 < rows[3]["seconds_kept"] < rows[1]["seconds_kept"]
    # the table, centre scan: without boxes the flash at 119 joins the run
    assert persist.main(common) == 0
    text = capsys.readouterr().out
    assert "centre scan" in text and "the longest has 30 motion frames" in text
    table = [ln.split() for ln in text.splitlines() if ln[:1].isdigit()]
    assert [int(r[0]) for r in table] == [1, 2, 3, 5] and [int(r[1]) for r in table] == [33, 30, 30, 30]
    assert "run lengths: 1: 3" in text
