"""GPU tier (`-m gpu`): the direction filter — sector votes and per-frame motion roses (include/mtgpu_dir.h,
csrc/dir_kernels.hip).

Every comparison is exact against tests/dir_model.py, which tests/test_dir_host.py ties to the unchanged oracle through
the record filter of consequence C and to the numbers written out by hand in tests/dir_inputs.py; consequence A is held
against mtgpu_scan_centres_device (existing code) bit for bit.  Outputs are pre-filled with junk: every element must be
written by the call."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, synth, tune

import dir_inputs as di
import dir_model as dm
from scan_checks import assert_counts_equal, device_centres_of, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG = -7, 9
NAMES = ("flags", "centres", "rose")


# ------------------------------------------------------------------ device helpers

def junk_outputs(n, pad=0):
    import torch
    return {"flags": torch.full((n + 2 * pad,), JUNK_FLAG, dtype=torch.uint8, device="cuda"),
            "centres": torch.full((n + 2 * pad,), JUNK, dtype=torch.int32, device="cuda"),
            "rose": torch.full((n + 2 * pad, 8), JUNK, dtype=torch.int32, device="cuda")}


def device_dir(s, d_rec, d_off, d_sd, compact, allow=0xFF, soff=None, allows=None, stream=None):
    """Through mtgpu_scan_dir_device into junk-filled outputs -> (flags uint8 [F], centres uint32 [F], rose uint32 [F, 8])
    on the host."""
    import torch
    n = d_off.numel() - 1
    out = junk_outputs(n)
    d_soff = None if soff is None else torch.from_numpy(np.asarray(soff).astype(np.int64)).cuda()
    d_allow = None if allows is None else torch.from_numpy(np.concatenate([np.asarray(allows, dtype=np.uint8), np.zeros(1, dtype=np.uint8)])).cuda()
    torch.cuda.synchronize()
    s.scan_dir_device(d_rec, d_off, d_sd, allow=allow, d_stream_off=d_soff, d_allow=d_allow, compact=compact, out=out, stream=stream)
    torch.cuda.synchronize()
    return (out["flags"].cpu().numpy(), out["centres"].cpu().numpy().view(np.uint32),
            out["rose"].cpu().numpy().view(np.uint32).reshape(n, 8))


def assert_equals_model(got, want, what):
    fl, ce, rose = got
    wfl, wce, wrose = want
    bad = np.flatnonzero((rose != wrose).any(axis=1))
    assert bad.size == 0, (f"{what}: the roses of {bad.size} of {len(wrose)} frames differ, first {bad[:6].tolist()}: "
                           f"want {wrose[bad[:6]].tolist()} got {rose[bad[:6]].tolist()}")
    assert_counts_equal(ce, wce, what, got_f=fl, want_f=wfl)


@functools.lru_cache(maxsize=None)
def model_of(name, allow=None):
    """The model's (flags, centres, rose) of a named case under its own streams, or under one byte: computed once."""
    c = CASES[name]()
    kw = dict(allow=c["allow"], soff=c["soff"], allows=c["allows"]) if allow is None else dict(allow=allow)
    return dm.model_batch(c["params"], c["mv"], c["off"], c["sd"], **kw)


CASES = dict(di.HAND_CASES, edge=di.edge_case, seam65=lambda: di.seam_case(65), seam129=lambda: di.seam_case(129), width=di.width_case,
             extreme=di.extreme_case, stream=di.stream_case)


def both_layouts(s, c, what, allow=None):
    """The case through the device entry point with both record sizes, under its own streams or one byte; yields
    (label, (flags, centres, rose))."""
    kw = dict(allow=c["allow"], soff=c["soff"], allows=c["allows"]) if allow is None else dict(allow=allow)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        assert d_rec.numel() == 0 or d_rec.data_ptr() % 128 == 0      # the phases of dir_inputs.edge_case rest on it
        yield f"{what}, {'compact' if compact else '40-byte'}", device_dir(s, d_rec, d_off, d_sd, compact, **kw)


# ------------------------------------------------------------------ 1. frames derived by hand

@pytest.mark.parametrize("name", sorted(di.HAND_CASES))
def test_hand_frames(gpu_scanner_factory, name):
    """The boundary points on the 6 x 5 grid under six allow bytes; a still record under threshold 0 and allow 0 votes
    and is in no bin; vectors_needed 0 (consequence F); a record in a margin row is in no bin and casts no vote."""
    c = CASES[name]()
    s = gpu_scanner_factory(c["params"])
    want = model_of(name)
    assert want[1].tolist() == c["hand_centres"].tolist() and want[2].tolist() == c["hand_rose"].tolist()
    for label, got in both_layouts(s, c, name):
        assert_equals_model(got, want, label)
    # the scalar form, stream by stream, and the host entry point
    for st, allow in enumerate(c["allows"].tolist()):
        a, b = int(c["soff"][st]), int(c["soff"][st + 1])
        for label, got in both_layouts(s, c, f"{name}, one byte {allow:#x}", allow=allow):
            assert got[1][a:b].tolist() == c["hand_centres"][a:b].tolist() and got[2][a:b].tolist() == c["hand_rose"][a:b].tolist(), label
    res = s.scan_dir(m.FrameBatch(c["mv"], c["off"], None, c["sd"]), stream_off=c["soff"], allows=c["allows"])
    assert_equals_model((res["flags"], res["centres"], res["rose"]), want, name + ", host entry")
    assert res["rose"].dtype == np.uint32 and res["rose"].shape == (len(c["sd"]), 8)


# ------------------------------------------------------------------ 2. the streamers' edges

def test_streamer_edges(gpu_scanner_factory):
    """Frames of 0, 1, 2, 15, 16, 17, 4095 .. 4097, 8191 .. 8193 and 8207 records, each starting on each of the sixteen
    8-byte phases of a 128-byte line, both record sizes; neighbouring records lie in different sectors, so a record
    dropped or read twice in the head peel, the odd tail or a partial step moves a bin."""
    c = CASES["edge"]()
    s = gpu_scanner_factory(c["params"])
    want = model_of("edge")
    assert want[2].tolist() == c["hand_rose"].tolist()
    for label, got in both_layouts(s, c, "streamer edges"):
        assert_equals_model(got, want, label)


EDGE_STREAM_ALLOWS = [0xA5, 0x0F, 0xFF]


def edge_streams(n_frames):
    """Three streams over the edge batch; its last five frames lie behind the last one."""
    return np.array([0, n_frames // 3, n_frames // 2, n_frames - 5], dtype=np.uint64)


def test_unaligned_40_byte_base(gpu_scanner_factory):
    """(base & 7) != 0 takes stream_mv40's branch without a head peel, here with dir_vote at 1024 lanes and four loads in
    flight: the edge batch (frames of 0 .. 8207 records, neighbouring records in different sectors, so a record skipped
    or read twice moves a bin) as 40-byte records at byte shifts 4, 12 and 20, under one byte and under one byte per
    stream — roses, centres and flags against the model.  An odd base is MT_ERR_INVALID and writes nothing: asserted here
    with a live context and junk-filled outputs (tests/api_arg_rungs.py holds the rung's place in the ladder, with a NULL
    context and made-up addresses)."""
    import torch
    from test_gpu_derived_edges import shifted
    from derived_edge_inputs import UNALIGNED_SHIFTS
    c = CASES["edge"]()
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    F = len(sd)
    s = gpu_scanner_factory(p)
    soff = edge_streams(F)
    wants = {"one byte": (dict(allow=c["allow"]), model_of("edge")),
             "per stream": (dict(soff=soff, allows=EDGE_STREAM_ALLOWS), dm.model_batch(p, mv, off, sd, soff=soff, allows=EDGE_STREAM_ALLOWS))}
    assert wants["one byte"][1][2].tolist() == c["hand_rose"].tolist() and not wants["per stream"][1][2][F - 5:].any()
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    _, d_off, d_sd = to_device(mv[:0], off, sd, False)
    for shift in UNALIGNED_SHIFTS:
        d_rec = shifted(raw, shift)
        for form, (kw, want) in wants.items():
            assert_equals_model(device_dir(s, d_rec, d_off, d_sd, False, **kw), want, f"base shifted by {shift} bytes, {form}")
    out = junk_outputs(F)
    odd = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")[1:1 + raw.numel()]
    rc = s._lib.mtgpu_scan_dir_device(s._ctx, odd.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), F, None, 0, None, 0xFF,
                                      out["flags"].data_ptr(), out["centres"].data_ptr(), out["rose"].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in s._lib.mtgpu_last_error().decode()
    assert all(int((t != (JUNK_FLAG if n == "flags" else JUNK)).sum()) == 0 for n, t in out.items())


# ------------------------------------------------------------------ 3. word seams

@pytest.mark.parametrize("gw", [65, 129])
def test_word_seams(gpu_scanner_factory, gw):
    """Allowed and forbidden records alternate across columns 63 | 64 (and 127 | 128): the centre pairs straddle the seam."""
    name = f"seam{gw}"
    c = CASES[name]()
    s = gpu_scanner_factory(c["params"])
    want = model_of(name)
    assert want[1].tolist() == di.SEAM_HAND[gw]
    for label, got in both_layouts(s, c, name):
        assert_equals_model(got, want, label)


# ------------------------------------------------------------------ 4. the width of the rose's counters

def test_counter_width(gpu_scanner_factory):
    """One frame of 300 000 records of sector 3 and one of each other sector: where packed per-lane counters go wrong."""
    c = CASES["width"]()
    s = gpu_scanner_factory(c["params"])
    want = model_of("width")
    hand = [1] * 8
    hand[di.WIDTH_SECTOR] = di.WIDTH_N
    assert want[2].tolist() == [hand]
    for label, got in both_layouts(s, c, "300 000 records"):
        assert got[2].tolist() == [hand], label
        assert_equals_model(got, want, label)
    for label, got in both_layouts(s, c, "300 000 records, all allowed", allow=0xFF):
        assert_equals_model(got, model_of("width", 0xFF), label)


# ------------------------------------------------------------------ 5. extremes

def test_extreme_displacements(gpu_scanner_factory):
    """+-65535 on each axis (the negative ones end outside the grid and do not count), (65535, 27306) E and (65535, 27307)
    SE, and their like on the west side: |d|^2 beyond 32 bits, products of the axis tests at their largest."""
    c = CASES["extreme"]()
    s = gpu_scanner_factory(c["params"])
    want = model_of("extreme")
    assert want[2].tolist() == [di.EXTREME_ROSE] * 2
    for label, got in both_layouts(s, c, "extremes"):
        assert_equals_model(got, want, label)


# ------------------------------------------------------------------ 6. streams

def test_streams(gpu_scanner_factory):
    """Streams of 0, 1, 2, 64, 0, 0 and 33 frames with different allow bytes; three frames in front of the first stream
    and five behind the last hold records and read 0 in outputs that start out non-zero; a key frame inside a stream;
    the scalar form on the same batch; the host entry point on the frames up to the last stream's end."""
    c = CASES["stream"]()
    s = gpu_scanner_factory(c["params"])
    want = model_of("stream")
    F = len(c["sd"])
    orphan = np.r_[0:di.STREAM_FRONT, F - di.STREAM_BEHIND:F]
    for label, got in both_layouts(s, c, "streams"):
        assert_equals_model(got, want, label)
        assert not got[0][orphan].any() and not got[1][orphan].any() and not got[2][orphan].any(), label
        k = di.STREAM_KEY_FRAME
        assert got[0][k] == 0 and got[1][k] == 0 and not got[2][k].any(), label
    one = model_of("stream", c["scalar_allow"])
    for label, got in both_layouts(s, c, "one byte for every frame", allow=c["scalar_allow"]):
        assert_equals_model(got, one, label)
    assert (one[1][orphan] > 0).any()                              # the same frames count under the scalar form
    n = F - di.STREAM_BEHIND
    res = s.scan_dir(m.FrameBatch(c["mv"][:int(c["off"][n])], c["off"][:n + 1], None, c["sd"][:n]), stream_off=c["soff"], allows=c["allows"])
    assert_equals_model((res["flags"], res["centres"], res["rose"]), tuple(w[:n] for w in want), "streams, host entry")
    with pytest.raises(m.MtgpuError) as ei:                        # the host entry point wants stream_off to end on n_frames
        s.scan_dir(m.FrameBatch(c["mv"], c["off"], None, c["sd"]), stream_off=c["soff"], allows=c["allows"])
    assert ei.value.code == _abi.MT_ERR_INVALID and "n_frames" in str(ei.value)


# ------------------------------------------------------------------ 7. the consequences on random draws

@pytest.mark.parametrize("i", range(di.N_DRAWS))
def test_consequences_on_random_draws(i):
    """Draw i (grids of the soak's set, vectors_needed i % 4, margin 0 .. 3, up to 12 frames of up to 3 000 records),
    compact records on odd draws.  A: allow = 0xFF is mtgpu_scan_centres_device bit for bit.  B: one rose under every
    allow, and its sum.  D: turned and mirrored records under the turned and mirrored byte.  E: a chain of growing
    bytes.  F where vectors_needed is 0.  Every output equals the model's."""
    c = di.draw(i)
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    compact = bool(i % 2)
    with m.MotionScanner(p, device=0) as s:
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        plain_f, plain_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        prev, first_rose = None, None
        for allow in di.DRAW_ALLOWS:
            got = device_dir(s, d_rec, d_off, d_sd, compact, allow=allow)
            assert_equals_model(got, dm.model_batch(p, mv, off, sd, allow=allow), f"draw {i} allow {allow:#x}")
            if first_rose is None:
                first_rose = got[2]
                assert first_rose.sum(axis=1).tolist() == dm.counting_moving(p, mv, off, sd).tolist()     # B
            assert np.array_equal(got[2], first_rose), f"draw {i}: the rose depends on allow {allow:#x}"   # B
            if prev is not None:
                assert (prev <= got[1]).all(), f"draw {i}: not monotone at allow {allow:#x}"               # E
            prev = got[1]
            if p.vectors_needed == 0:
                assert_counts_equal(got[1], plain_c, f"draw {i} vn 0 allow {allow:#x}", got_f=got[0], want_f=plain_f)   # F
            if allow in (0x1B, 0x5B):                                                                      # D
                for turn, perm, other in ((di.rotated, lambda k: (k + 2) & 7, direction.rotate_allow(allow, 2)),
                                          (di.mirrored, lambda k: (4 - k) & 7, direction.mirror_allow(allow))):
                    t_rec, _, _ = to_device(turn(mv), off, sd, compact)
                    fl2, ce2, rose2 = device_dir(s, t_rec, d_off, d_sd, compact, allow=other)
                    assert_counts_equal(ce2, got[1], f"draw {i} allow {allow:#x} -> {other:#x}", got_f=fl2, want_f=got[0])
                    assert np.array_equal(rose2[:, [perm(k) for k in range(8)]], got[2])
        assert_counts_equal(prev, plain_c, f"draw {i}: allow 0xFF against the centre scan", got_f=got[0], want_f=plain_f)   # A


# ------------------------------------------------------------------ 8. refusals and exact writes

def test_refusals_touch_nothing_and_the_next_call_succeeds(gpu_scanner_factory):
    """Every MT_ERR_INVALID / MT_ERR_UNSUPPORTED of the device entry point with a live context: the argument is named,
    canaries on both sides of every output and the outputs themselves are untouched, and the call that follows succeeds.
    Then every combination of NULL outputs, n_frames == 0 and a non-default stream."""
    import torch
    c = CASES["stream"]()
    p, mv, off, sd, soff, allows = c["params"], c["mv"], c["off"], c["sd"], c["soff"], c["allows"]
    want = dict(zip(NAMES, model_of("stream")))
    s = gpu_scanner_factory(p)
    lib = s._lib
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_soff = torch.from_numpy(soff.astype(np.int64)).cuda()
    d_allow = torch.from_numpy(allows.copy()).cuda()
    F, PAD = len(off) - 1, 64

    def run(names=NAMES, n_frames=F, rb=8, stream=None, ctx=None, over=None, so=True, ns=None, al=True, allow=0, off_ptr=None):
        b = junk_outputs(F, PAD)
        torch.cuda.synchronize()
        ptr = {n: (b[n][PAD:].data_ptr() if n in names else None) for n in NAMES}
        ptr.update(over or {})
        rc = lib.mtgpu_scan_dir_device((ctx or s)._ctx, d_rec.data_ptr(), rb, len(mv), d_off.data_ptr() if off_ptr is None else off_ptr,
                                       d_sd.data_ptr(), n_frames, d_soff.data_ptr() if so else None,
                                       (len(soff) - 1 if so and al else 0) if ns is None else ns, d_allow.data_ptr() if al else None,
                                       allow, ptr["flags"], ptr["centres"], ptr["rose"], stream)
        torch.cuda.synchronize()
        return rc, {n: t.cpu().numpy() for n, t in b.items()}, lib.mtgpu_last_error().decode()

    def untouched(raw, names=NAMES):
        return all((raw[n] == (JUNK_FLAG if n == "flags" else JUNK)).all() for n in names)

    def good(raw, names=NAMES):
        for n in NAMES:
            junk = JUNK_FLAG if n == "flags" else JUNK
            assert (raw[n][:PAD] == junk).all() and (raw[n][PAD + F:] == junk).all(), (names, n)
            if n in names:
                got = raw[n][PAD:PAD + F]
                assert np.array_equal(got if n == "flags" else got.view(np.uint32), want[n]), (names, n)
            else:
                assert untouched(raw, (n,)), (names, n)

    def refused(code, word, **kw):
        rc, raw, msg = run(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert untouched(raw), kw
        rc, raw, msg = run()                                        # the next call succeeds
        assert rc == _abi.MT_OK, msg
        good(raw)

    inv = _abi.MT_ERR_INVALID
    for allow in (-1, 256):
        refused(inv, "allow", allow=allow)                          # in range even where d_allow is given
        refused(inv, "allow", allow=allow, so=False, al=False)
    for rb in (0, 16, 41):
        refused(inv, "rec_bytes", rb=rb)
    refused(inv, "all NULL", names=())
    refused(inv, "d_frame_off is NULL", off_ptr=0)
    refused(inv, "d_frame_off must be 8-byte aligned", off_ptr=d_off.data_ptr() + 4)
    refused(inv, "d_stream_off is NULL", so=False, ns=7)
    refused(inv, "n_streams is 0", ns=0)
    refused(inv, "d_allow is NULL", al=False)                       # d_stream_off given
    refused(inv, "d_allow is NULL", al=False, so=False, ns=7)       # n_streams given
    pinned = torch.full((F * 8,), JUNK, dtype=torch.int32).pin_memory()
    for name in NAMES:
        refused(inv, "d_" + name + " is not memory of device", over={name: pinned.data_ptr()})
        assert int((pinned != JUNK).sum()) == 0
    refused(inv, "d_centres must be 4-byte aligned", over={"centres": junk_outputs(F)["centres"].data_ptr() + 2})
    refused(inv, "d_rose must be 4-byte aligned", over={"rose": junk_outputs(F)["rose"].data_ptr() + 1})
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    refused(_abi.MT_ERR_UNSUPPORTED, "960x540", ctx=big)
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_dir(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # every combination of NULL outputs
    for names in [NAMES, ("flags", "centres"), ("flags", "rose"), ("centres", "rose"), ("flags",), ("centres",), ("rose",)]:
        rc, raw, msg = run(names)
        assert rc == _abi.MT_OK, (names, msg)
        good(raw, names)
    # n_frames == 0: MT_OK, nothing written
    rc, raw, msg = run(n_frames=0)
    assert rc == _abi.MT_OK and untouched(raw)
    res = s.scan_dir(m.FrameBatch(mv[:0], off[:1], None, None))
    assert len(res["flags"]) == len(res["centres"]) == 0 and res["rose"].shape == (0, 8)
    # a non-default stream
    st = torch.cuda.Stream()
    rc, raw, msg = run(stream=st.cuda_stream)
    assert rc == _abi.MT_OK, msg
    good(raw)


def test_contract_program_in_c(tmp_path):
    """tests/c/abi_dir_canaries.c: the caller-sized buffers exactly as the header sizes them, from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_dir_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_dir_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all direction buffers respected" in out.stdout


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    c = CASES["stream"]()
    s = gpu_scanner_factory(c["params"])
    d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_dir(s, d_rec, d_off, d_sd, False, soff=c["soff"], allows=c["allows"])
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert_equals_model(got, model_of("stream"), "profiled call")


def test_has_sd_null_and_a_window_of_a_batch(gpu_scanner_factory):
    """has_sd == NULL: side data iff records; offsets that do not start at 0 through the host entry point."""
    c = CASES["stream"]()
    p, mv, off = c["params"], c["mv"], c["off"]
    s = gpu_scanner_factory(p)
    want = dm.model_batch(p, mv, off, None, allow=0x5B)
    d_rec, d_off, _ = to_device(mv, off, None, True)
    assert_equals_model(device_dir(s, d_rec, d_off, None, True, allow=0x5B), want, "has_sd NULL, device entry")
    res = s.scan_dir(m.FrameBatch(mv, off, None, None), allow=0x5B)
    assert_equals_model((res["flags"], res["centres"], res["rose"]), want, "has_sd NULL, host entry")
    a, b = 20, 50
    res = s.scan_dir(m.FrameBatch(mv, off[a:b + 1], None, None), allow=0x5B)
    assert_equals_model((res["flags"], res["centres"], res["rose"]), tuple(w[a:b] for w in want), "a window, host entry")


# ------------------------------------------------------------------ 9. end to end

@pytest.fixture(scope="module")
def two_events():
    """50 frames of a 1080p stream at 25 fps: an object that moves east in frames 5 .. 14, one that moves west in frames
    32 .. 41, apart in time; key frames without side data at 0 and 30; no salt cells, no records outside the picture."""
    spec = synth.spec_1080p(seed=3, sub=1, salt_p=0.0, oob_p=0.0)
    spec.events = [synth.Event(5, 15, 30, 30, 4, 3, 9, 0), synth.Event(32, 42, 70, 20, 4, 3, -9, 0)]
    F = 50
    frames = [synth.gen_frame(spec, f) for f in range(F)]
    return F, frames


def test_end_to_end_command(gpu_scanner_factory, two_events, tmp_path):
    """A .mtmv written with mvfile, then `python -m mvtrim_amd.direction --json` in a fresh child process with each of
    the two ignore masks and --each: the model decides the expected frame sets; the two masks keep different, non-empty
    sets; the segments come from the unchanged merge."""
    F, frames = two_events
    path = str(tmp_path / "street.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1)
    batch, pts, hdr = tune.load(path)
    assert batch.n_frames == F
    mv, off, sd = np.ascontiguousarray(batch.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(batch.frame_off, dtype=np.uint64), batch.has_sd
    no_west, no_east = 0xFF & ~direction.allow_from_names("W,NW,SW"), 0xFF & ~direction.allow_from_names("E,NE,SE")
    sets = {}
    for allow in (0xFF, no_west, no_east):
        fl, ce, rose = dm.model_batch(p, mv, off, sd, allow=allow)
        sets[allow] = set(np.flatnonzero(fl).tolist())
    assert sets[no_west] == set(range(5, 15)) and sets[no_east] == set(range(32, 42)) and sets[0xFF] == sets[no_west] | sets[no_east]
    s = gpu_scanner_factory(p)
    for allow in sets:
        assert set(np.flatnonzero(s.scan_dir(batch, allow=allow)["flags"]).tolist()) == sets[allow]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "mvtrim_amd.direction", path, "--json", "--vectors-needed", "1", "--max-gap-sec", "0.2",
            "--padding-sec", "0.04", "--min-savings-pct", "5"]
    docs = {}
    for names in ("W,NW,SW", "E,NE,SE"):
        out = subprocess.run(base + ["--ignore", names] + (["--each"] if names[0] == "W" else []), capture_output=True, text=True,
                             env=env, cwd=ROOT, timeout=300)
        assert out.returncode == 0, out.stderr
        docs[names] = json.loads(out.stdout)
    west, east = docs["W,NW,SW"], docs["E,NE,SE"]
    assert west["all"] == east["all"] and west["all"]["motion_frames"] == 20 and west["all"]["segments"] == 2
    assert west["mask"]["motion_frames"] == 10 and west["mask"]["segments"] == 1 and west["mask"]["sectors"] == "E,SE,S,N,NE"
    assert east["mask"]["motion_frames"] == 10 and east["mask"]["segments"] == 1 and east["mask"]["allow"] == no_east
    assert 0.0 < west["mask"]["seconds_kept"] < west["all"]["seconds_kept"] < F / 25.0
    fl, ce, rose = dm.model_batch(p, mv, off, sd, allow=0xFF)
    assert [t["records"] for t in west["rose"]] == rose.sum(axis=0).tolist()
    assert [t["records_kept"] for t in west["rose"]] == rose[fl != 0].sum(axis=0).tolist()
    assert west["rose"][0]["records_kept"] == west["rose"][4]["records_kept"] > 0 and abs(sum(t["share"] for t in west["rose"]) - 1.0) < 1e-9
    # --each: the wedge around E takes the first object, the wedge around W the second, the wedge around S neither
    each = {r["ignored"]: r for r in west["each"]}
    assert len(each) == 8 and each["E,SE,NE"]["motion_frames"] == 10 == each["SW,W,NW"]["motion_frames"] and each["SE,S,SW"]["motion_frames"] == 20
    # the table, in this process
    assert direction.main(base[3:4] + base[5:] + ["--allow", "E"]) == 0


def test_plain_c_dir_example(tmp_path):
    """examples/dir_example.c: a car with the traffic, a walker against it, from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "dir_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "dir_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all                  20 frames kept, 2 segment(s)" in out.stdout
    assert "--ignore W,NW,SW     10 frames kept, 1 segment(s)" in out.stdout
    assert "--ignore E,NE,SE     10 frames kept, 1 segment(s)" in out.stdout
    assert "rose of frame 15: E 6, W 0; of frame 45: E 0, W 4" in out.stdout
