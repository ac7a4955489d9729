"""How many scan workgroups share a CU is a launch parameter (the size of the dynamic LDS: choose_lds_floor, mtgpu_api.hip),
chosen per launch — one per CU for launches of large 40-byte frames — and forced by MTGPU_WG_PER_CU.  It must never
change a result.  The 512-thread single-tile kernels over 40-byte records (32-bit counters, the 1-bit field, CAS8) against
the oracle, flags AND centre counts, on a 1080p grid with the code defaults and the shipped env, at whatever the tile
allows (three per CU), at two and at one per CU: more than 1024 ragged frames in one launch, frame sizes around a
streaming step, every phase of a 128-byte line for the first record; and the automatic choice on a launch that meets
its condition.  Inputs are built on the host once per parameter set and shared by the forms."""
import functools

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import synth

import oracle_binding as ob
from scan_checks import assert_centres_parity, junk_padding

pytestmark = pytest.mark.gpu

STEP = 4 * 512                     # records of one streaming step: 4 loads in flight per lane, 512 lanes
SIZES = [0, 1, 15, 16, 17, STEP - 1, STEP, STEP + 1, 2 * STEP + 15]

# (name, parameter set, vectors_needed override, MTGPU_FORCE_FB, counter bits, counter mode)
FORMS = [("add32-code", "code_defaults", None, None, 32, 0),
         ("add32-env", "shipped_env", None, None, 32, 0),
         ("or1-code", "code_defaults", 1, 1, 1, 1),
         ("cas8-code", "code_defaults", None, 108, 8, 2),
         ("cas8-env", "shipped_env", None, 108, 8, 2)]
FORM_IDS = [f[0] for f in FORMS]


def config_of(cfg, vec):
    kw = dict(m.config.CODE_DEFAULTS if cfg == "code_defaults" else m.config.SHIPPED_ENV)
    if vec is not None:
        kw["vectors_needed"] = vec
    return kw


PER_CU = [-1, 2, 1]               # MTGPU_WG_PER_CU: what the tile allows / at most two / one


def scanner_of(factory, form, per_cu, monkeypatch):
    name, cfg, vec, force_fb, fb, mode = form
    kw = config_of(cfg, vec)
    p = ob.params_from_config(1920, 1080, **kw)
    assert (p.grid_w, p.grid_h) == (120, 68)
    monkeypatch.setenv("MTGPU_WG_PER_CU", str(per_cu))      # read at create time
    s = factory(p, force_fb=force_fb, force_block=512)
    monkeypatch.delenv("MTGPU_WG_PER_CU")
    plan = s.plan
    assert (plan["block_threads"], plan["bands"], plan["counter_bits"], plan["counter_mode"]) == (512, 1, fb, mode), plan
    assert plan["lds_bytes"] <= 40 * 1024, plan          # the tile itself would fit a CU four times
    return s, p, kw


def planted_frame(n, vec, at_head, rng):
    """n records, all but min(n, 2 vec) of them at rest somewhere in the frame; those vote, alternately, for the
    adjacent cells (50, 30) and (51, 30) and are the FIRST (at_head) or the LAST records of the frame: with 2 vec or
    more records both cells are active, each the other's neighbour — 2 centres — and only if every one of the first /
    last records was scanned."""
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["dst_x"] = rng.randint(0, 1920, size=n)
    mv["dst_y"] = rng.randint(0, 1080, size=n)
    mv["src_x"], mv["src_y"] = mv["dst_x"], mv["dst_y"]
    k = min(n, 2 * vec)
    idx = np.arange(k) if at_head else np.arange(n - k, n)
    mv["dst_x"][idx] = 16 * (50 + np.arange(k) % 2) + rng.randint(0, 16, size=k)
    mv["dst_y"][idx] = 16 * 30 + rng.randint(0, 16, size=k)
    mv["src_x"][idx], mv["src_y"][idx] = mv["dst_x"][idx] - 7, mv["dst_y"][idx]
    return junk_padding(mv, rng)


def batch_of(frames, sd):
    counts = np.array([len(f) for f in frames], dtype=np.uint64)
    off = np.zeros(len(frames) + 1, dtype=np.uint64)
    np.cumsum(counts, out=off[1:])
    mv = np.concatenate(frames) if frames else np.zeros(0, dtype=m.MV_DTYPE)
    return mv, off, np.asarray(sd, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def ragged_case(cfg, vec):
    """About 1100 small ragged frames, empty frames and frames without side data among them, and the oracle's answer."""
    rng = np.random.RandomState(2200 + (vec or 0))
    mv, off, sd = synth.random_frames(rng, 1100, 500, 1920, 1080, hot=0.5)
    junk_padding(mv, rng)
    p = ob.params_from_config(1920, 1080, **config_of(cfg, vec))
    want = ob.scan_centres(p, mv, off, sd)
    for a in (mv, off, sd) + tuple(want):
        a.setflags(write=False)
    return mv, off, sd, want


@functools.lru_cache(maxsize=None)
def sizes_case(cfg, vec):
    """Frames of SIZES records, votes at the head and at the tail, in a shuffled order (so that they start at different
    places of a 128-byte line), with an empty frame that has side data, one that has none, and a voting frame without
    side data; the oracle's centre counts equal the ones that follow from the construction."""
    kw = config_of(cfg, vec)
    v = kw["vectors_needed"]
    rng = np.random.RandomState(4100 + v)
    frames, sd, hand = [], [], []
    for n in SIZES:
        for at_head in (True, False):
            frames.append(planted_frame(n, v, at_head, rng))
            sd.append(1)
            hand.append(2 if n >= 2 * v else 0)          # fewer: at most one of the two cells is active
    frames.append(planted_frame(STEP + 9, v, False, rng)); sd.append(0); hand.append(0)      # no side data: never motion
    frames.append(np.zeros(0, dtype=m.MV_DTYPE)); sd.append(0); hand.append(0)
    order = rng.permutation(len(frames))
    frames, sd, hand = [frames[i] for i in order], [sd[i] for i in order], [hand[i] for i in order]
    mv, off, sd = batch_of(frames, sd)
    p = ob.params_from_config(1920, 1080, **kw)
    want = ob.scan_centres(p, mv, off, sd)
    assert want[1].tolist() == hand
    assert np.array_equal(want[0], (want[1] >= kw["clusters_needed"]).astype(np.uint8))
    assert 0 < want[0].sum() < len(want[0])
    for a in (mv, off, sd) + tuple(want):
        a.setflags(write=False)
    return mv, off, sd, want


@functools.lru_cache(maxsize=None)
def phase_case(cfg, vec, r0, first_n):
    """A batch whose records start r0 records into the array — 40 r0 mod 128 takes each of the 16 eight-byte phases of
    a line for r0 = 0 .. 15 — and whose first frame votes with its FIRST records (the ones stream_mv40 hands to lanes
    0 .. h-1 ahead of the aligned stream; first_n = 3 is shorter than most h).  Returns the whole array, the offsets
    of the window behind the r0 records, and the oracle's answer for the window."""
    kw = config_of(cfg, vec)
    v = kw["vectors_needed"]
    rng = np.random.RandomState(7000 + 100 * r0 + first_n + v)
    frames = [planted_frame(r0, v, True, rng), planted_frame(first_n, v, True, rng)]
    frames += [planted_frame(int(n), v, bool(i % 2), rng) for i, n in enumerate(rng.randint(1, 2 * STEP + 200, size=5))]
    mv, off, sd = batch_of(frames, [1] * len(frames))
    off, sd = off[1:].copy(), sd[1:].copy()
    p = ob.params_from_config(1920, 1080, **kw)
    want = ob.scan_centres(p, mv, off, sd)
    if first_n >= 2 * v:
        assert want[1][0] == 2
    for a in (mv, off, sd) + tuple(want):
        a.setflags(write=False)
    return mv, off, sd, want


def check(s, p, case, what):
    mv, off, sd, want = case
    got = s.check_frames(m.FrameBatch(mv, off, None, sd))
    assert np.array_equal(got, want[0]), (what, np.flatnonzero(got != want[0])[:8].tolist(), s.plan)
    assert_centres_parity(s, p, mv, off, sd, plain_flags=got, want=want, device=True, what=what)


@pytest.mark.parametrize("per_cu", PER_CU)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_ragged_frames_beyond_every_slot(gpu_scanner_factory, monkeypatch, form, per_cu):
    """More than 1024 frames in one launch: every workgroup slot of the chip is taken and reused, at any residency."""
    s, p, _ = scanner_of(gpu_scanner_factory, form, per_cu, monkeypatch)
    case = ragged_case(form[1], form[2])
    assert len(case[2]) > 1024
    assert 0 < case[3][0].sum() < len(case[2]) and (case[2] == 0).any() and (np.diff(case[1].astype(np.int64)) == 0).any()
    check(s, p, case, f"{form[0]} ragged, per CU {per_cu}")


@pytest.mark.parametrize("per_cu", PER_CU)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_frame_sizes_around_a_streaming_step(gpu_scanner_factory, monkeypatch, form, per_cu):
    s, p, _ = scanner_of(gpu_scanner_factory, form, per_cu, monkeypatch)
    check(s, p, sizes_case(form[1], form[2]), f"{form[0]} sizes, per CU {per_cu}")


@pytest.mark.parametrize("per_cu", PER_CU)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_every_line_phase_of_the_first_frame(gpu_scanner_factory, monkeypatch, form, per_cu):
    s, p, _ = scanner_of(gpu_scanner_factory, form, per_cu, monkeypatch)
    for r0 in range(16):
        for first_n in (3, 40):
            check(s, p, phase_case(form[1], form[2], r0, first_n), f"{form[0]} phase {r0} first frame {first_n}, per CU {per_cu}")


@pytest.mark.parametrize("cfg", ["code_defaults", "shipped_env"])
def test_automatic_choice_on_a_launch_of_large_frames(gpu_scanner_factory, monkeypatch, cfg):
    """A launch that meets choose_lds_floor's condition — 40-byte frames of 1.3 MB, more than eight per CU — on a scanner
    with no knob set, next to the same launch with the choice switched off: flags and centre counts equal each other's
    and the oracle's, frame for frame (the batch is 60 generated frames, tiled on the device)."""
    import torch
    from scan_checks import device_centres_of
    kw = config_of(cfg, None)
    spec = synth.spec_1080p(seed=31, sub=2)
    spec.events = synth.scripted_events(spec, 60)
    mv, off, _, sd = synth.gen_stream(spec, 60)
    p = ob.params_from_config(1920, 1080, **kw)
    want_f, want_c = ob.scan_centres(p, mv, off, sd)
    assert 0 < want_f.sum() < 60 and (sd == 0).any()
    monkeypatch.delenv("MTGPU_WG_PER_CU", raising=False)
    auto = gpu_scanner_factory(p)
    cus = auto.plan["cu_count"]
    reps = (8 * cus + 59) // 60 + 1
    frames = 60 * reps
    counts = np.tile(np.diff(off.astype(np.int64)), reps)
    assert frames >= 8 * cus and 40 * counts.sum() // frames >= 512 * 1024
    d_mv = torch.from_numpy(mv.view(np.uint8).copy()).cuda().repeat(reps)
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).cuda()
    d_sd = torch.from_numpy(np.tile(sd, reps)).cuda()
    monkeypatch.setenv("MTGPU_WG_PER_CU", "-1")
    off_ = gpu_scanner_factory(p)
    monkeypatch.delenv("MTGPU_WG_PER_CU")
    for s in (auto, off_):
        assert (s.plan["block_threads"], s.plan["counter_bits"], s.plan["bands"]) == (512, 32, 1)
        fl, ce = device_centres_of(s, d_mv, d_off, d_sd, compact=False)
        assert np.array_equal(fl, np.tile(want_f, reps)) and np.array_equal(ce, np.tile(want_c, reps).astype(np.uint32))
        plain = s.check_frames_device(d_mv, d_off, d_sd)
        torch.cuda.synchronize()
        assert np.array_equal(plain.cpu().numpy(), np.tile(want_f, reps))
