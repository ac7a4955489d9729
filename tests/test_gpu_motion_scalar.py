"""GPU tier (`-m gpu`): the per-second motion scalar (tools/motion_scalar.cpp:61-84) — per-frame scores and per-second
bins — against the oracle's mto_motion_scalar, against sequential sums of the GPU's own per-frame scores, and against
the stdout of the reference's own tool (tests/golden/motion_scalar_golden.json, reference_live_vectors.json).

Tolerances.  u = 2^-53; n = the number of addends behind a value (its terms, plus its frames for a bin).  Terms are
bit-identical on both sides and >= 0, so two summation orders of the same n addends differ by at most
2 * gamma(n-1) * S <= (2n + 2) * u * S.  Where a sum is exact in every order (integer terms) or has one addend, the
comparison is on the bits."""
import ctypes as C
import importlib.util
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, synth

import oracle_binding as ob

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -53
# one pass of a motion_scores_kernel workgroup: kScoresBlock (512) lanes x kScoresUnroll (4) records (csrc/scalar_kernels.h)
PASS = 512 * 4
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, PASS - 1, PASS, PASS + 1, 40000]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def scanner(gpu_scanner_factory):
    return gpu_scanner_factory(m.ScanParams.from_config(1920, 1080))


def upload(mv, off):
    import torch
    mv = np.ascontiguousarray(mv, dtype=m.MV_DTYPE)
    d_mv = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy()).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    return d_mv, d_off


def gpu_scores(s, mv, off, **kw):
    import torch
    d_mv, d_off = upload(mv, off)
    sc, tm = s.motion_scores_device(d_mv, d_off, **kw)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), (None if tm is None else tm.cpu().numpy().view(np.uint32))


def oracle_scores(mv, off):
    """Per-frame sums from the oracle: one frame per second."""
    n = len(off) - 1
    return ob.motion_scalar(mv, off, np.arange(n, dtype=np.float64), n)


def count_terms(mv, off):
    nz = np.concatenate([[0], np.cumsum(mv["motion_scale"] != 0)])
    o = np.asarray(off).astype(np.int64)
    return (nz[o[1:]] - nz[o[:-1]]).astype(np.uint32)


def offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    np.cumsum(sizes, out=off[1:])
    return off


# ------------------------------------------------------------------ 1. terms

def test_single_terms_are_bit_exact(scanner):
    """4096 frames of one record each: with one addend there is no summation order, so every score must have the
    bits the CPU computes — division by every kind of scale (powers of two take the reciprocal path), the square
    root, the two products."""
    rng = np.random.RandomState(1)
    n = 4096
    scales = np.array([1, 2, 3, 4, 7, 16, 255, 65535], dtype=np.uint16)
    hard = [(3, 4), (0, 0), (-2 ** 31, -2 ** 31), (2 ** 31 - 1, 1)]
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["motion_scale"] = scales[np.arange(n) % 8]
    mv["motion_x"] = rng.randint(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    mv["motion_y"] = rng.randint(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    small = slice(n // 2, n)
    mv["motion_x"][small] = rng.randint(-64, 65, size=n // 2)
    mv["motion_y"][small] = rng.randint(-64, 65, size=n // 2)
    mv["w"] = rng.randint(0, 256, size=n)
    mv["h"] = rng.randint(0, 256, size=n)
    mv["w"][:256], mv["h"][:256] = np.arange(256), np.arange(256)[::-1]
    for i, (x, y) in enumerate(hard):                    # every hard pair with every scale, on non-trivial blocks
        at = slice(512 + 8 * i, 520 + 8 * i)
        mv["motion_x"][at], mv["motion_y"][at] = x, y
        mv["w"][at], mv["h"][at] = 16, 8
    # the other fields of a record must not matter
    mv["src_x"], mv["dst_y"], mv["flags"], mv["source"] = -1, 32767, 2 ** 64 - 1, -1
    off = np.arange(n + 1, dtype=np.uint64)
    got, terms = gpu_scores(scanner, mv, off)
    want = oracle_scores(mv, off)
    bad = np.nonzero(bits(got) != bits(want))[0]
    print("single terms: mismatches", len(bad), [(int(i), mv[i], got[i], want[i]) for i in bad[:5]])
    assert len(bad) == 0
    assert want[512] == 5.0 * 16 * 8 and want[513] == 2.5 * 16 * 8 and np.isfinite(want).all() and want.max() > 1e12
    assert terms.tolist() == [1] * n


# ------------------------------------------------------------------ 2. integer-valued frames

def integer_frames(rng, sizes):
    pairs = np.array([(3, 4), (-5, 12), (8, -15), (20, 21), (0, 7), (0, 0)])
    total = int(sum(sizes))
    mv = np.zeros(total, dtype=m.MV_DTYPE)
    pick = rng.randint(0, len(pairs), size=total)
    mv["motion_x"], mv["motion_y"] = pairs[pick, 0], pairs[pick, 1]
    mv["w"] = 2 ** rng.randint(0, 5, size=total)
    mv["h"] = 2 ** rng.randint(0, 5, size=total)
    mv["motion_scale"] = (rng.random_sample(total) >= 0.2).astype(np.uint16)      # about 20 % are skipped
    return mv, offsets(sizes)


@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_integer_frames_are_bit_exact_at_every_size(scanner, order):
    """Every term is an integer below 2^13, every sum exact in any order: bits equal the oracle's at every frame size
    around the wave, the workgroup, one workgroup pass (PASS) and far above; frames follow each other directly, so
    most start off a 128-byte line."""
    sizes = SIZES if order == "ascending" else SIZES[::-1]
    mv, off = integer_frames(np.random.RandomState(2), sizes)
    got, terms = gpu_scores(scanner, mv, off)
    want = oracle_scores(mv, off)
    print(order, "scores", got.tolist())
    assert want.max() < 2 ** 53 and (want == np.floor(want)).all() and (want[np.array(sizes) > 2] > 0).all()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(terms, count_terms(mv, off)) and terms.sum() < len(mv)


# ------------------------------------------------------------------ 3. general values

def general_frames(rng, sizes):
    total = int(sum(sizes))
    mv = np.zeros(total, dtype=m.MV_DTYPE)
    mv["motion_x"] = rng.randint(-2 ** 15, 2 ** 15 + 1, size=total)
    mv["motion_y"] = rng.randint(-2 ** 15, 2 ** 15 + 1, size=total)
    mv["w"] = rng.randint(1, 256, size=total)
    mv["h"] = rng.randint(1, 256, size=total)
    mv["motion_scale"] = 4
    return mv, offsets(sizes)


def assert_within_bound(got, want, n, what):
    got, want, n = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(n, dtype=np.float64)
    err = np.abs(got - want)
    bound = (2.0 * n + 2.0) * U * want
    worst = int(np.argmax(err - bound))
    print(what, "max err / bound", float(np.max(err / np.maximum(bound, 1e-300))), "worst", worst, got[worst], want[worst], n[worst])
    assert (err <= bound).all(), (what, worst, got[worst], want[worst], n[worst])


def test_general_frames_are_within_the_derived_bound(scanner):
    mv, off = general_frames(np.random.RandomState(3), SIZES)
    got, terms = gpu_scores(scanner, mv, off)
    want = oracle_scores(mv, off)
    assert np.array_equal(terms, np.array(SIZES, dtype=np.uint32))
    assert_within_bound(got, want, terms, "general frames")
    assert got[0] == 0.0 and not np.signbit(got[0])
    assert bits(got[1]) == bits(want[1])                    # one addend


# ------------------------------------------------------------------ 4. reproducible

def test_same_call_same_bits(scanner):
    import torch
    mv, off = general_frames(np.random.RandomState(4), SIZES[::-1])
    d_mv, d_off = upload(mv, off)
    a, ta = scanner.motion_scores_device(d_mv, d_off)
    b, tb = scanner.motion_scores_device(d_mv, d_off)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    c, tc = scanner.motion_scores_device(d_mv, d_off, stream=st.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))
    assert torch.equal(ta, tb) and torch.equal(ta, tc)


# ------------------------------------------------------------------ 5. bins

@pytest.fixture(scope="module")
def bin_batch(scanner):
    """Three streams of 0, 1 and 2500 small frames, their GPU scores (computed once, shared) and unsorted timestamps."""
    rng = np.random.RandomState(5)
    stream_off = np.array([0, 0, 1, 2501], dtype=np.int64)
    sizes = rng.randint(0, 40, size=2501)
    sizes[::97] = 0
    mv, off = general_frames(rng, sizes)
    mv["motion_scale"][rng.random_sample(len(mv)) < 0.1] = 0
    scores, terms = gpu_scores(scanner, mv, off)
    return mv, off, stream_off, scores, terms


@pytest.mark.parametrize("n_sec", [1, 7, 5000])
def test_bins(scanner, bin_batch, n_sec):
    import torch
    mv, off, stream_off, scores, terms = bin_batch
    rng = np.random.RandomState(50 + n_sec)
    n = len(scores)
    pts = rng.random_sample(n) * n_sec * 1.25                # unsorted; a fifth lie at or past n_sec
    pts[rng.random_sample(n) < 0.05] = -1.0                  # null
    pts[rng.random_sample(n) < 0.02] = -1e-9
    pts[rng.random_sample(n) < 0.03] = float("nan")
    pts[7], pts[8], pts[9] = float(n_sec), n_sec - 2.0 ** -40, float("inf")
    pts[0] = 0.5                                             # the one-frame stream lands in bin 0
    d = [torch.from_numpy(x).cuda() for x in (scores, terms.view(np.int32), pts, stream_off)]
    acc, bt = scanner.motion_bins_device(d[0], d[1], d[2], d[3], n_sec)
    torch.cuda.synchronize()
    acc, bt = acc.cpu().numpy(), bt.cpu().numpy()
    assert acc.shape == (3, n_sec) and bt.shape == (3, n_sec)
    skipped = 0
    for s in range(3):
        want = [0.0] * n_sec                                 # sequential Python sums of the GPU's own scores, in frame order
        want_t, frames_in = [0] * n_sec, [0] * n_sec
        for f in range(int(stream_off[s]), int(stream_off[s + 1])):
            p = float(pts[f])
            if not (p >= 0.0) or math.isinf(p) or math.floor(p) >= n_sec:
                skipped += 1
                continue
            b = int(math.floor(p))
            want[b] += float(scores[f])
            want_t[b] += int(terms[f])
            frames_in[b] += 1
        assert np.array_equal(bits(acc[s]), bits(np.array(want))), (s, n_sec)     # a property of the kernel, no tolerance
        assert bt[s].tolist() == want_t
        assert not np.signbit(acc[s]).any()
        f0, f1 = int(stream_off[s]), int(stream_off[s + 1])
        ref = ob.motion_scalar(mv, off[f0:f1 + 1], np.where(np.isfinite(pts[f0:f1]), pts[f0:f1], -1.0), n_sec)
        assert_within_bound(acc[s], ref, np.array(want_t) + np.array(frames_in), "bins of stream %d, n_sec %d" % (s, n_sec))
    assert skipped > 300 and acc[0].tolist() == [0.0] * n_sec and bt[0].sum() == 0 and bt[1, 0] == terms[0]


# ------------------------------------------------------------------ 6. the reference's own output

def golden_streams():
    spec_ = importlib.util.spec_from_file_location("mk", os.path.join(GOLD, "make_motion_scalar_golden.py"))
    mk = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mk)
    spec, frames, pts = mk.build()
    rows = json.load(open(os.path.join(GOLD, "motion_scalar_golden.json")))["rows"]
    yield "golden", spec, frames, pts, [(int(a), b) for a, b in rows]
    spec = synth.StreamSpec(width=320, height=240, block=16, sub=1, fps=30.0, gop=10, seed=9, salt_p=0.05)
    spec.events = [synth.Event(3, 40, 4, 3, 5, 4, 11, -7)]
    frames = [synth.gen_frame(spec, i) for i in range(70)]
    pts = [spec.pts_seconds(i) for i in range(70)]
    rows = json.load(open(os.path.join(GOLD, "reference_live_vectors.json")))["motion_scalar"]["rows"]
    yield "live", spec, frames, pts, [(int(a), b) for a, b in rows]


def close_to_gold(value, gold_text, n):
    gold = float(gold_text)
    return abs(value - gold) <= 5e-6 * gold + (2 * n + 2) * U * gold


def run_command(path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.motion_scalar", path], capture_output=True, text=True,
                         env=env, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


def test_against_the_reference_tools_own_output(scanner, tmp_path):
    """Expected values printed by object code compiled from the reference's tools/motion_scalar.cpp: the same set of
    seconds, every value within the golden strings' own precision (six significant digits: half a unit of the sixth)
    plus the summation bound.  Then the command, on the JSON and on the .mtmv container."""
    for name, spec, frames, pts, gold in golden_streams():
        pts6 = [float("%.6f" % p) for p in pts]                 # the JSON carries %.6f seconds
        batch = m.FrameBatch.from_frames(frames)
        acc, bt = scanner.motion_scalar(batch, pts6)
        seconds = [int(s) for s in np.nonzero(bt)[0]]
        print(name, "seconds", seconds, "acc", acc.tolist(), "gold", gold)
        assert seconds == [s for s, _ in gold]
        assert seconds == ([0, 1, 2, 3] if name == "golden" else [0, 1, 2])
        frames_in = np.bincount(np.floor(pts6).astype(int), minlength=len(acc))
        n_of = {s: int(bt[s]) + int(frames_in[s]) for s in seconds}
        for s, text in gold:
            assert close_to_gold(float(acc[s]), text, n_of[s]), (name, s, acc[s], text)
        js, mt = str(tmp_path / (name + ".json")), str(tmp_path / (name + ".mtmv"))
        m.mvjson.write_json(js, frames, pts, (1, spec.tb_den))
        m.mvfile.write_mtmv(mt, spec.width, spec.height, 1, spec.tb_den, spec.fps, len(frames) / spec.fps,
                            [spec.pts_ticks(i) for i in range(len(frames))], frames)
        for path in (js, mt):
            lines = run_command(path)
            assert lines[0] == "second,motion_value" and len(lines) == 1 + len(gold), lines
            for ln, (s, text) in zip(lines[1:], gold):
                a, b = ln.split(",")
                assert int(a) == s and close_to_gold(float(b), text, n_of[s]), (name, path, ln, text)


# ------------------------------------------------------------------ 7. buffers

GUARD = 16


def test_guards_null_outputs_and_pinned_memory(scanner):
    import torch
    lib = m.load_library()
    mv, off = general_frames(np.random.RandomState(7), [0, 5, 0, 700, 64, 0, PASS + 3, 1, 0])
    n = len(off) - 1
    d_mv, d_off = upload(mv, off)
    st = torch.cuda.current_stream().cuda_stream
    want, want_t = gpu_scores(scanner, mv, off)
    assert want_t.tolist() == [0, 5, 0, 700, 64, 0, PASS + 3, 1, 0] and want[0] == 0.0

    def guarded(count, dtype, fill, pinned=False):
        t = torch.full((count + 2 * GUARD,), fill, dtype=dtype)
        return t.pin_memory() if pinned else t.cuda()

    def check(t, count, fill, inner=None):
        a = t.cpu().numpy()
        assert (a[:GUARD] == fill).all() and (a[GUARD + count:] == fill).all(), "guard overwritten"
        if inner is not None:
            assert np.array_equal(a[GUARD:GUARD + count], inner)
        return a[GUARD:GUARD + count]

    NANBITS = -2251799813685248          # 0xFFF8000000000000: compared as int64 so that the fill can be told from results
    for pinned in (False, True):
        sc = guarded(n, torch.int64, NANBITS, pinned)
        tm = guarded(n, torch.int32, -7, pinned)
        _abi.check(lib.mtgpu_motion_scores_device(scanner._ctx, d_mv.data_ptr(), len(mv), d_off.data_ptr(), n,
                                                  sc.data_ptr() + 8 * GUARD, tm.data_ptr() + 4 * GUARD, st))
        torch.cuda.synchronize()
        check(sc, n, NANBITS, bits(want))
        check(tm, n, -7, want_t.view(np.int32))
        # d_terms == NULL: the doubles only
        sc2 = guarded(n, torch.int64, NANBITS, pinned)
        _abi.check(lib.mtgpu_motion_scores_device(scanner._ctx, d_mv.data_ptr(), len(mv), d_off.data_ptr(), n,
                                                  sc2.data_ptr() + 8 * GUARD, None, st))
        torch.cuda.synchronize()
        check(sc2, n, NANBITS, bits(want))
        # the bins: 2 streams x 5 seconds
        n_sec, soff = 5, torch.tensor([0, 4, n], dtype=torch.int64).cuda()
        pts = torch.tensor([0.0, 1.5, 1.25, 9.0, 4.9, -1.0, 0.1, 0.2, 3.0], dtype=torch.float64).cuda()
        d_sc, d_tm = torch.from_numpy(want).cuda(), torch.from_numpy(want_t.view(np.int32)).cuda()
        acc = guarded(2 * n_sec, torch.int64, NANBITS, pinned)
        bt = guarded(2 * n_sec, torch.int64, -9, pinned)
        _abi.check(lib.mtgpu_motion_bins_device(scanner._ctx, d_sc.data_ptr(), d_tm.data_ptr(), pts.data_ptr(), soff.data_ptr(),
                                                2, n_sec, acc.data_ptr() + 8 * GUARD, bt.data_ptr() + 8 * GUARD, st))
        torch.cuda.synchronize()
        want_acc = np.array([0.0, want[1] + want[2], 0, 0, 0, want[6] + want[7], 0, 0, want[8], want[4]])
        check(acc, 2 * n_sec, NANBITS, bits(want_acc))
        check(bt, 2 * n_sec, -9, np.array([0, 5, 0, 0, 0, PASS + 4, 0, 0, 0, 64]))
        acc2 = guarded(2 * n_sec, torch.int64, NANBITS, pinned)
        _abi.check(lib.mtgpu_motion_bins_device(scanner._ctx, d_sc.data_ptr(), None, pts.data_ptr(), soff.data_ptr(),
                                                2, n_sec, acc2.data_ptr() + 8 * GUARD, None, st))
        torch.cuda.synchronize()
        check(acc2, 2 * n_sec, NANBITS, bits(want_acc))


def test_arguments_are_checked_before_anything_is_launched(scanner):
    import torch
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    mv, off = general_frames(np.random.RandomState(8), [3, 4])
    d_mv, d_off = upload(mv, off)
    sc = torch.full((4,), 9.0, dtype=torch.float64).cuda()
    tm = torch.full((4,), -7, dtype=torch.int32).cuda()
    pts = torch.zeros(2, dtype=torch.float64).cuda()
    soff = torch.tensor([0, 2], dtype=torch.int64).cuda()
    ctx = scanner._ctx

    def err():
        return lib.mtgpu_last_error().decode()

    assert lib.mtgpu_motion_scores_device(ctx, d_mv.data_ptr(), 7, None, 2, sc.data_ptr(), None, None) == inv and "d_frame_off" in err()
    assert lib.mtgpu_motion_scores_device(ctx, d_mv.data_ptr(), 7, d_off.data_ptr(), 2, None, tm.data_ptr(), None) == inv
    assert lib.mtgpu_motion_scores_device(ctx, None, 7, d_off.data_ptr(), 2, sc.data_ptr(), None, None) == inv and "d_mv" in err()
    assert lib.mtgpu_motion_scores_device(ctx, d_mv.data_ptr(), 7, d_off.data_ptr(), 2, sc.data_ptr() + 4, None, None) == inv
    assert lib.mtgpu_motion_bins_device(ctx, sc.data_ptr(), tm.data_ptr(), pts.data_ptr(), soff.data_ptr(), 1, 0, sc.data_ptr(), None, None) == inv
    assert "n_sec" in err()
    assert lib.mtgpu_motion_bins_device(ctx, sc.data_ptr(), tm.data_ptr(), None, soff.data_ptr(), 1, 2, sc.data_ptr(), None, None) == inv
    assert lib.mtgpu_motion_bins_device(ctx, sc.data_ptr(), None, pts.data_ptr(), soff.data_ptr(), 1, 2, sc.data_ptr(), tm.data_ptr(), None) == inv
    # the host entry point: NULL outputs, n_sec == 0, decreasing offsets
    h_off = np.array([0, 4, 3], dtype=np.uint64)
    h_pts, acc = np.zeros(2), np.full(2, 9.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                          # noqa: E731
    assert lib.mtgpu_motion_scalar(ctx, p(mv), p(h_off), p(h_pts), 2, 2, p(acc), None) == inv and "monotonic" in err()
    h_off[2] = 7
    assert lib.mtgpu_motion_scalar(ctx, p(mv), p(h_off), p(h_pts), 2, 0, p(acc), None) == inv and "n_sec" in err()
    assert lib.mtgpu_motion_scalar(ctx, p(mv), p(h_off), p(h_pts), 2, 2, None, None) == inv
    assert lib.mtgpu_motion_scalar(ctx, p(mv), p(h_off), None, 2, 2, p(acc), None) == inv
    assert lib.mtgpu_motion_scalar(ctx, None, p(h_off), p(h_pts), 2, 2, p(acc), None) == inv
    torch.cuda.synchronize()
    assert sc.cpu().tolist() == [9.0] * 4 and tm.cpu().tolist() == [-7] * 4 and acc.tolist() == [9.0, 9.0]
    # and the call that is right: host entry point == device entry points on the same records
    _abi.check(lib.mtgpu_motion_scalar(ctx, p(mv), p(h_off), p(h_pts), 2, 2, p(acc), None))
    want = oracle_scores(mv, h_off)
    assert_within_bound(acc, [want.sum(), 0.0], [9, 0], "host entry point")
    scores, terms = scanner.motion_scores(m.FrameBatch(mv, h_off))
    assert terms.dtype == np.uint32 and terms.tolist() == [4, 3]
    assert_within_bound(scores, want, terms, "motion_scores")


# ------------------------------------------------------------------ 8. the example

def test_plain_c_motion_scalar_example(tmp_path):
    """examples/motion_scalar_example.c: the activity curve of a tiny stream from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "motion_scalar_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "motion_scalar_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.splitlines() == ["second,motion_value", "0,3200", "2,19200"]
