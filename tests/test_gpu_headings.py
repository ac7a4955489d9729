"""GPU tier (`-m gpu`): object headings — the rose and the summed displacement of every listed object
(include/mtgpu_headings.h, csrc/headings_kernels.hip).

Expected values: the numbers written out by hand in tests/headings_inputs.py; the numpy restatement
tests/headings_model.py (composed from blobs_model, objects_model, dir_model and direction.sector_of) elsewhere;
mtgpu_scan_objects_device and mtgpu_scan_dir_device (existing code) on the same device buffers for consequences A, B and
D.  tests/test_headings_host.py holds the model and the hand values against each other without a GPU.  Every comparison
is exact; outputs are pre-filled with junk: every element must be written by the call.  The cases run from the smallest
grid to the largest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, headings, objects, tune

import blobs_inputs as bi
import headings_inputs as hi
import headings_model as hm
import objects_inputs as oi
import test_gpu_blobs as tb
import test_gpu_objects as to
import zones_inputs as zi
from derived_edge_inputs import voters
from scan_checks import to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = headings.OUTPUTS
JUNK, JUNK_FLAG = -7, 9
WORDS = headings.HEADING_WORDS


# ------------------------------------------------------------------ device helpers

def junk_outputs(n, k, want=OUTPUTS):
    import torch
    out = {}
    for name in want:
        shape = {"list": (n, k, 4), "motion": (n, k, WORDS)}.get(name, (n,))
        out[name] = torch.full(shape, JUNK_FLAG if name == "flags" else JUNK, dtype=torch.uint8 if name == "flags" else torch.int32, device="cuda")
    return out


def to_host(res):
    out = {}
    for name, t in res.items():
        if t is not None:
            a = t.cpu().numpy()
            out[name] = (a if name == "flags" else a.view(hm.om.OBJECT_DTYPE)[..., 0] if name == "list" else
                         a.view(hm.HEADING_DTYPE)[..., 0] if name == "motion" else a.view(np.uint32))
    return out


def device_headings(s, d_rec, d_off, d_sd, compact, k=16, min_blob=1, min_objects=1, allow=0xFF, d_soff=None, d_keep=None, want=OUTPUTS):
    """Through mtgpu_scan_headings_device into junk-filled outputs -> {name: numpy array} on the host."""
    import torch
    out = junk_outputs(d_off.numel() - 1, k, want)
    torch.cuda.synchronize()
    res = headings.scan_device(s, d_rec, d_off, d_sd, k, min_blob, min_objects, allow, d_soff, d_keep, compact=compact, want=want, out=out)
    torch.cuda.synchronize()
    return to_host(res)


def layout_name(compact):
    return "compact" if compact else "40-byte"


def assert_outputs(got, want, what, p=None, min_objects=1):
    """got: the call's outputs; want: headings_model.model_batch's dict (or headings_inputs.hand_want's).  Exact."""
    for name in ("centres", "blobs", "objects", "allowed"):
        if name in want:
            assert got[name].tolist() == np.asarray(want[name]).tolist(), (what, name, got[name].tolist(), np.asarray(want[name]).tolist())
    assert hm.same(got["list"], want["list"]), (what, "list", got["list"], want["list"])
    if not hm.same(got["motion"], want["motion"]):
        bad = np.argwhere((got["motion"].view(np.uint8).reshape(got["motion"].shape + (64,)) !=
                           want["motion"].view(np.uint8).reshape(want["motion"].shape + (64,))).any(axis=-1))
        f, j = bad[0]
        raise AssertionError(f"{what}: motion of {len(bad)} entries differs, first frame {f} entry {j}: want {want['motion'][f, j]} "
                             f"got {got['motion'][f, j]}")
    assert (got["motion"]["reserved"] == 0).all(), what
    if p is not None and "allowed" in want:
        wf = hm.flags_np(p, want["centres"], want["allowed"], min_objects)
        assert got["flags"].tolist() == wf.tolist(), (what, "flags", got["flags"].tolist(), wf.tolist())


def assert_identities(got, what, p):
    """Consequence D's first two lines, the empties, and the heading rule."""
    mo, lst = got["motion"], got["list"]
    n = mo["n"].astype(np.int64)
    rec, cells = mo["records"].astype(np.int64), lst["cells"].astype(np.int64)
    assert (n.sum(axis=-1) <= rec).all(), what
    if 1 <= (p.vectors_needed & 0xFF) <= 255:
        assert (rec >= cells * (p.vectors_needed & 0xFF)).all(), what
    empty = cells == 0
    assert (rec[empty] == 0).all() and (n[empty] == 0).all() and (mo["heading"][empty] == hm.NONE).all(), what
    assert (mo["sum_dx"][empty] == 0).all() and (mo["sum_dy"][empty] == 0).all(), what
    best = n.max(axis=-1)
    head = np.where(best > 0, n.argmax(axis=-1), hm.NONE)           # argmax: the first, i.e. the lowest sector
    assert (mo["heading"].astype(np.int64) == head).all(), what


def object_scan(s, d_rec, d_off, d_sd, compact, k, min_blob, min_objects, d_soff, d_keep):
    return to.device_objects(s, d_rec, d_off, d_sd, compact, k, min_blob, min_objects, d_soff, d_keep)


def assert_consequences_a_b(got, obj, what, with_flags):
    for name in ("centres", "blobs", "objects"):
        assert got[name].tolist() == obj[name].tolist(), (what, "A", name)
    assert hm.same(got["list"], obj["list"]), (what, "A", "list")
    if with_flags:                      # allow == 0xFF
        k = got["list"].shape[1]
        assert got["allowed"].tolist() == np.minimum(obj["objects"], k).tolist(), (what, "B", "allowed")
        assert got["flags"].tolist() == obj["flags"].tolist(), (what, "B", "flags")


# ------------------------------------------------------------------ 1. three blobs on the smallest grid, by hand

@pytest.mark.parametrize("thr", [16, 0])
@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "masks"])
def test_three_blobs_by_hand(gpu_scanner_factory, thr, masked):
    """63 x 12, margin 1: a blob all E, a blob with a 2 : 2 tie between W and NE (heading W, the lower sector), and — at
    threshold 0 only — a blob of still records (heading NONE, always allowed); around them a slow record inside a blob
    cell, a record in an active column-0 cell, one in an isolated active cell, one in a margin row and one out of bounds,
    which belong to no entry.  k = 1, 2, 3, 16, every hand value of `allowed`; each output alone; the host entry point."""
    p, mv, off, sd, soff, keeps = hi.hand_case(thr)
    s = gpu_scanner_factory(p)
    d_soff, d_keep = (tb.soff_tensor(soff), tb.keep_tensor(keeps)) if masked else (None, None)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        full = device_headings(s, d_rec, d_off, d_sd, compact, 16, 1, 1, 0xFF, d_soff, d_keep)
        for k in (1, 2, 3, 16):
            for (t, allow, mbc) in hi.HAND_ALLOWED:
                if t != thr:
                    continue
                for mo in (1, min(2, k)):
                    what = f"hand, thr {thr}, {layout_name(compact)}, k {k}, allow {allow:#x}, min_blob_cells {mbc}, min_objects {mo}"
                    got = device_headings(s, d_rec, d_off, d_sd, compact, k, mbc, mo, allow, d_soff, d_keep)
                    assert_outputs(got, hi.hand_want(thr, k, mbc, allow, masked), what, p, mo)
                    assert_identities(got, what, p)
                    assert hm.same(got["motion"], full["motion"][:, :k]) and hm.same(got["list"], full["list"][:, :k]), what    # C
        # each output alone: the six others are not asked for
        ref = device_headings(s, d_rec, d_off, d_sd, compact, 3, 3, 2, 1 << hi.E, d_soff, d_keep)
        for name in OUTPUTS:
            one = device_headings(s, d_rec, d_off, d_sd, compact, 3, 3, 2, 1 << hi.E, d_soff, d_keep, want=(name,))
            assert list(one) == [name] and hm.same(one[name], ref[name]), name
    # the host entry point (its stream table ends at the batch's last frame: the first three frames under the mask)
    F = 3 if masked else 4
    r = headings.scan(s, m.FrameBatch(mv, off[:F + 1], None, sd[:F]), 3, 1, 2, 1 << hi.W, *((soff, zi.pack_keeps(keeps)) if masked else ()))
    want = {n: v[:F] for n, v in hi.hand_want(thr, 3, 1, 1 << hi.W, masked).items()}
    assert_outputs(r, want, "host entry", p, 2)
    assert r["motion"].dtype == headings.HEADING_DTYPE and r["motion"].shape == (F, 3) and r["list"].shape == (F, 3)
    mean = headings.mean_vector(r["motion"])
    assert mean.shape == (F, 3, 2) and mean[0, 0].tolist() == [31 / 4, 6 / 4] and mean[1].tolist() == [[0.0, 0.0]] * 3


def test_the_hand_case_as_one_stream_of_four(gpu_scanner_factory):
    """Four streams under keep masks — a random one, the hand frames, an empty one, a random one: the hand stream's
    answers are the hand numbers, and the whole batch is the model's."""
    p, mv, off, sd, _, _ = hi.hand_case(0)
    rng = np.random.RandomState(5)
    fr = lambda lo, hi_: [None if not sd[f] else mv[int(off[f]):int(off[f + 1])] for f in range(lo, hi_)]      # noqa: E731
    noise = [voters([(int(rng.randint(1, 62)), int(rng.randint(1, 11)), 2, int(rng.randint(-9, 9)), int(rng.randint(-9, 9))) for _ in range(40)])
             for _ in range(3)]
    bmv, boff, bsd = bi.batch_of(noise[:2] + fr(0, 4) + noise[2:], 71)
    soff = np.array([0, 2, 6, 6, 7], dtype=np.uint64)
    keeps = np.ones((4, hi.HAND_GH, hi.HAND_GW), dtype=bool)
    keeps[0] = rng.rand(hi.HAND_GH, hi.HAND_GW) > 0.2
    s = gpu_scanner_factory(p)
    want = hm.model_batch(p, bmv, boff, bsd, 3, 1, 1 << hi.E, soff, keeps)
    hand = hi.hand_want(0, 3, 1, 1 << hi.E)
    for n in hand:
        assert hm.same(want[n][2:6], hand[n]), n
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(bmv, boff, bsd, compact)
        got = device_headings(s, d_rec, d_off, d_sd, compact, 3, 1, 1, 1 << hi.E, tb.soff_tensor(soff), tb.keep_tensor(keeps))
        assert_outputs(got, want, f"one stream of four, {layout_name(compact)}", p, 1)


# ------------------------------------------------------------------ 2. more blobs than entries

def test_seventeen_blobs_at_k_1_2_15_16(gpu_scanner_factory):
    """120 x 68, 17 blobs of 18 .. 2 cells, blob i moving in sector i & 7: at every k the records of the unlisted blobs
    are in no entry, and motion for k is the head of motion for 16 (C)."""
    p, mv, off, sd = hi.seventeen_case()
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for k in (16, 15, 2, 1):
            what = f"seventeen, {layout_name(compact)}, k {k}"
            got = device_headings(s, d_rec, d_off, d_sd, compact, k, 4, k, 0x0F)
            assert hm.same(got["motion"], hi.seventeen_motion(k)), (what, got["motion"])
            assert_outputs(got, hm.model_batch(p, mv, off, sd, k, 4, 0x0F), what, p, k)
            assert int(got["motion"]["records"].sum()) == sum(18 - i for i in range(k)) and got["blobs"].tolist() == [17], what
        # headings 0 .. 3 are allowed: blobs 0 .. 3 and 8 .. 11 of the 15 with at least 4 cells
        assert got["objects"].tolist() == [15]
        assert device_headings(s, d_rec, d_off, d_sd, compact, 16, 4, 8, 0x0F)["allowed"].tolist() == [8]
        assert device_headings(s, d_rec, d_off, d_sd, compact, 16, 4, 9, 0x0F)["flags"].tolist() == [0]
        assert device_headings(s, d_rec, d_off, d_sd, compact, 16, 4, 8, 0x0F)["flags"].tolist() == [1]


# ------------------------------------------------------------------ 3. word seams

def test_word_seams_with_a_direction_per_blob(gpu_scanner_factory):
    """2000 x 9: bars across the column-64, 128 and 1024 seams and a blob of 38 cells, each with its own direction: the
    hand entries at k = 16, 4 and 2."""
    p, mv, off, sd, hand = hi.seams_case()
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for k in (16, 4, 2):
            what = f"seams, {layout_name(compact)}, k {k}"
            got = device_headings(s, d_rec, d_off, d_sd, compact, k, 12, 2, (1 << hi.N) | (1 << hi.SE))
            assert hm.same(got["motion"], hi.motion_of(hand, k)[None]), (what, got["motion"])
            assert hm.same(got["list"], oi.om.entries(oi.SEAM_LIST, k)[None]), what
            assert got["allowed"].tolist() == [2 if k > 2 else 1] and got["flags"].tolist() == [int(k > 2)], what


# ------------------------------------------------------------------ 4. one frame of 40 000 records

@pytest.mark.parametrize("compact", [False, True], ids=["40-byte", "compact"])
def test_forty_thousand_records_of_the_largest_dx(gpu_scanner_factory, compact):
    """One blob of two cells takes 40 000 records with dx = 65535: sum_dx = 40 000 * 65 535 > 2^31; the stream loop's
    head, steps and tail all run; the 40-byte records begin at byte 120 — 8-byte aligned, not 128-byte aligned."""
    p, mv, off, sd = hi.big_case()
    s = gpu_scanner_factory(p)
    d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
    assert d_rec.data_ptr() % 128 == 0 and int(off[1]) * 40 % 128 == 120
    got = device_headings(s, d_rec, d_off, d_sd, compact, 2)
    want_m = np.stack([hm.empty_motion(2), hi.motion_of([hi.BIG_MOTION], 2)])
    want_l = np.stack([oi.om.entries([], 2), oi.om.entries([hi.BIG_LIST], 2)])
    assert hm.same(got["motion"], want_m), got["motion"]
    assert hm.same(got["list"], want_l) and got["allowed"].tolist() == [0, 1] and got["flags"].tolist() == [0, 1]
    assert int(got["motion"]["sum_dx"][1, 0]) == 40000 * 65535 > 2 ** 31


# ------------------------------------------------------------------ 5. masks and streams

def test_seventy_streams_and_a_mask_that_splits_a_blob(gpu_scanner_factory):
    """70 streams over 96 frames, empty and one-frame streams among them, frames without side data, frames behind
    stream_off[n_streams]; stream 1's keep plane clears one column through the middle of a bar, which splits it in two.
    Against the model, both record forms; A and B against the object scan on the same buffers."""
    p = bi.grid(120, 68, margin=3)
    rng = np.random.RandomState(11)
    step = [(6, 0), (6, 6), (0, 6), (-6, 6), (-6, 0), (-6, -6), (0, -6), (6, -6)]
    frames = []
    for f in range(96):
        if f % 7 == 3:
            frames.append(None)
            continue
        cells = []
        for i in range(int(rng.randint(0, 4))):
            d = step[int(rng.randint(0, 8))]
            cells += [(20 + j, 8 + 9 * i, 2) + d for j in range(int(rng.randint(2, 12)))]
        cells += [(int(rng.randint(0, 120)), int(rng.randint(0, 68)), 1, 5, 0) for _ in range(6)]
        frames.append(voters(cells))
    frames[1] = voters([(20 + j, 8, 2, 6, 0) for j in range(9)])                 # the bar the mask splits: 4 + 4 cells
    mv, off, sd = bi.batch_of(frames, 72)
    cuts = sorted(set([0, 1, 2, 2, 90]) | set(rng.choice(np.arange(3, 90), 65, replace=False).tolist()))
    soff = np.array(sorted(cuts + [2, 40]), dtype=np.uint64)                     # two empty streams
    assert len(soff) == 71 and int(soff[-1]) == 90 < 96
    keeps = rng.rand(70, 68, 120) >= 0.05
    keeps[1] = True
    keeps[1, :, 24] = False
    want = hm.model_batch(p, mv, off, sd, 4, 2, 0x11, soff, keeps)
    assert want["blobs"][1] == 2 and want["list"]["cells"][1, :2].tolist() == [4, 4] and want["motion"]["records"][1, :2].tolist() == [8, 8]
    assert (want["blobs"][90:] == 0).all() and want["blobs"][:90].max() >= 2
    s = gpu_scanner_factory(p)
    d_soff, d_keep = tb.soff_tensor(soff), tb.keep_tensor(keeps)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        what = f"70 streams, {layout_name(compact)}"
        got = device_headings(s, d_rec, d_off, d_sd, compact, 4, 2, 1, 0x11, d_soff, d_keep)
        assert_outputs(got, want, what, p, 1)
        assert_identities(got, what, p)
        assert_consequences_a_b(got, object_scan(s, d_rec, d_off, d_sd, compact, 4, 2, 1, d_soff, d_keep), what, False)
        alls = device_headings(s, d_rec, d_off, d_sd, compact, 4, 2, 2, 0xFF, d_soff, d_keep)
        assert_consequences_a_b(alls, object_scan(s, d_rec, d_off, d_sd, compact, 4, 2, 2, d_soff, d_keep), what, True)
        assert hm.same(alls["motion"], got["motion"]), what                      # C: motion does not depend on allow / min_objects


# ------------------------------------------------------------------ 6. the cliff

@pytest.mark.parametrize("k", [16, 1])
def test_last_grid_the_preview_accepts(gpu_scanner_factory, k):
    """The tallest 65-column grid the preview accepts for k entries: twenty runs up from the last row, each with its own
    direction, both record forms, against the model; the motion table ends at the last byte the launch asks for.  One
    more row is refused by both entry points with the grid named and no output byte touched."""
    import torch
    p, mv, off, sd = hi.cliff_case(k)
    gh = hi.cliff_rows(k)
    assert headings.preview(p, k)["lds_bytes"] == hi.lds_by_hand(65, gh, k) <= hi.MI355X_LDS < hi.lds_by_hand(65, gh + 1, k)
    want = hm.model_batch(p, mv, off, sd, k, 5, 0x0F)
    assert want["blobs"].tolist() == [20] and int(want["motion"]["records"][0, 0]) == 21
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        what = f"cliff 65x{gh}, k {k}, {layout_name(compact)}"
        got = device_headings(s, d_rec, d_off, d_sd, compact, k, 5, 1, 0x0F)
        assert_outputs(got, want, what, p, 1)
        assert_identities(got, what, p)
    if k == 16:
        p2 = bi.limit_params(65, gh + 1, vectors_needed=1, clusters_needed=1)
        assert hi.preview_or_none(p2, 16) is None
        s2 = gpu_scanner_factory(p2)
        d_rec, d_off, d_sd = to_device(mv, off, sd, False)
        out = junk_outputs(1, 16)
        fresh = to_host(junk_outputs(1, 16))
        with pytest.raises(m.MtgpuError) as ei:
            headings.scan_device(s2, d_rec, d_off, d_sd, 16, out=out)
        torch.cuda.synchronize()
        assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and f"65x{gh + 1}" in str(ei.value)
        after = to_host(out)
        for name in OUTPUTS:
            assert after[name].tobytes() == fresh[name].tobytes(), name
        with pytest.raises(m.MtgpuError) as ei:
            headings.scan(s2, m.FrameBatch(mv, off, None, sd), 16)
        assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and f"65x{gh + 1}" in str(ei.value)


# ------------------------------------------------------------------ 7. random draws; A, B, D, E, F

@pytest.mark.parametrize("seed", range(16))
def test_random_draws_all_seven_outputs(gpu_scanner_factory, seed):
    """Small random grids, thresholds 0 / 4 / 16, still and slow records, with and without masks, both record forms: all
    seven outputs are the model's; A and B against the object scan, D against the direction scan, on the same buffers."""
    p, mv, off, sd, soff, keeps = hi.random_case(seed)
    s = gpu_scanner_factory(p)
    k, mbc, mo, allow = (1, 2, 5, 16)[seed % 4], 1 + seed % 3, 1 + (seed % 2 if seed % 4 else 0), (0xFF, 0x0F, 0xA5, 0x00)[(seed // 4) % 4]
    for masked in (False, True):
        d_soff, d_keep = (tb.soff_tensor(soff), tb.keep_tensor(keeps)) if masked else (None, None)
        want = hm.model_batch(p, mv, off, sd, k, mbc, allow, soff if masked else None, keeps if masked else None)
        for compact in (False, True):
            d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
            what = f"draw {seed} {p.grid_w}x{p.grid_h}, {layout_name(compact)}, masked {masked}, k {k}"
            got = device_headings(s, d_rec, d_off, d_sd, compact, k, mbc, mo, allow, d_soff, d_keep)
            assert_outputs(got, want, what, p, mo)
            assert_identities(got, what, p)
            assert_consequences_a_b(got, object_scan(s, d_rec, d_off, d_sd, compact, k, mbc, mo, d_soff, d_keep), what, allow == 0xFF)
            if not masked:          # D: per sector, the entries' records are among the frame's counting records
                rose = s.scan_dir_device(d_rec, d_off, d_sd, compact=compact, want=("rose",))["rose"].cpu().numpy().view(np.uint32)
                assert (got["motion"]["n"].astype(np.int64).sum(axis=1) <= rose).all(), what


def test_rose_equality_and_the_quarter_turn(gpu_scanner_factory):
    """D: a frame in which every counting record lands in a listed blob — the entries' bins sum to the direction scan's
    rose exactly.  E: every src replaced by dst - (-dy, dx): the list stays, n turns by two sectors, the sums turn, and
    the heading turns where the maximum is unique."""
    p = hi.with_threshold(bi.grid(120, 68, margin=3, vn=2), 4.0)
    rng = np.random.RandomState(21)
    cells = []
    for i in range(5):
        for j in range(3 + 2 * i):
            for y in (10 + 8 * i, 11 + 8 * i):
                cells += [(30 + j, y, 1, int(rng.randint(-9, 10)), int(rng.randint(-9, 10))) for _ in range(3)]
    cells = [c if c[3] ** 2 + c[4] ** 2 >= 4 else c[:3] + (3, -1) for c in cells]
    mv, off, sd = bi.batch_of([voters(cells)], 73)
    s = gpu_scanner_factory(p)
    tmv = hm.quarter_turn(mv)
    want, twant = hm.model_batch(p, mv, off, sd, 16), hm.model_batch(p, tmv, off, sd, 16)
    assert want["blobs"].tolist() == [5] and int(want["motion"]["records"].sum()) == len(mv)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        got = device_headings(s, d_rec, d_off, d_sd, compact, 16)
        assert_outputs(got, want, "equality frame", p, 1)
        rose = s.scan_dir_device(d_rec, d_off, d_sd, compact=compact, want=("rose",))["rose"].cpu().numpy().view(np.uint32)
        assert (got["motion"]["n"].astype(np.int64).sum(axis=1) == rose).all() and int(rose.sum()) == len(mv)
        t_rec, t_off, t_sd = to_device(tmv, off, sd, compact)
        tgot = device_headings(s, t_rec, t_off, t_sd, compact, 16)
        assert_outputs(tgot, twant, "turned frame", p, 1)
        exp = hm.turned(got["motion"])
        assert hm.same(tgot["list"], got["list"])
        for name in ("n", "records", "sum_dx", "sum_dy"):
            assert np.array_equal(tgot["motion"][name], exp[name]), name
        u = hm.unique_max(got["motion"])
        assert u.any() and np.array_equal(tgot["motion"]["heading"][u], exp["heading"][u])


def test_allowed_through_the_sweep_is_flags_through_the_merge(gpu_scanner_factory):
    """F: allow a subset of allow' gives allowed <= allowed'; with clusters_needed 1, three streams, levels 1, 2, 4:
    mtgpu_sweep_streams_device on `allowed` == mtgpu_merge_streams_device on flags at min_objects = L, byte for byte."""
    import torch
    p, mv, off, sd, pts, soff = oi.streams_case()
    mv = mv.copy()
    flip = np.arange(len(mv)) % 3 == 0               # a third of the records point W instead of E
    mv["src_x"][flip] = mv["dst_x"][flip] + 5
    s = gpu_scanner_factory(p)
    CAP = 16
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_pts, d_soff = torch.from_numpy(pts.copy()).cuda(), tb.soff_tensor(soff)
    mps = [m.MergeParams(duration=oi.STREAM_FRAMES / oi.FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0) for _ in range(oi.STREAMS)]
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    levels = list(oi.SWEEP_LEVELS)
    allow = 1 << hi.E
    res = headings.scan_device(s, d_rec, d_off, d_sd, 16, oi.SWEEP_MIN_BLOB, 1, allow, compact=True)
    allowed = res["allowed"].cpu().numpy().view(np.uint32)
    want = hm.model_batch(p, mv, off, sd, 16, oi.SWEEP_MIN_BLOB, allow)
    assert allowed.tolist() == want["allowed"].tolist() and 0 < int(allowed.sum()) < int(want["objects"].sum())
    prev = np.zeros_like(allowed)
    for byte in (0, allow, allow | (1 << hi.W), 0xFF):
        nxt = device_headings(s, d_rec, d_off, d_sd, True, 16, oi.SWEEP_MIN_BLOB, 1, byte, want=("allowed",))["allowed"]
        assert (prev <= nxt).all(), byte
        prev = nxt
    assert prev.tolist() == want["objects"].tolist()
    sseg, sres = s.sweep_streams_device(res["allowed"], d_pts, d_soff, d_mp, levels, seg_cap=CAP)
    torch.cuda.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)        # noqa: E731
    for li, lv in enumerate(levels):
        fl = headings.scan_device(s, d_rec, d_off, d_sd, 16, oi.SWEEP_MIN_BLOB, lv, allow, compact=True, want=("flags",))["flags"]
        seg, r8 = s.merge_streams_device(fl, d_pts, d_soff, d_mp, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg.cpu().numpy())), lv
        assert np.array_equal(sres[li].cpu().numpy(), r8.cpu().numpy()), lv
        assert int(fl.sum()) == int((allowed >= lv).sum()), lv


# ------------------------------------------------------------------ 8. the refusals of the device entry point

def test_refusals_leave_the_outputs_alone(gpu_scanner_factory):
    """min_objects above k, allow out of range, a misaligned or host-resident motion array: refused with the argument
    named, junk untouched; then the same buffers serve a good call."""
    import torch
    p, mv, off, sd, _, _ = hi.hand_case(16)
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    out = junk_outputs(4, 4)
    host_motion = np.full((4, 4, WORDS), JUNK, dtype=np.int32)

    def call(k, min_objects, allow, mot):
        rc = lib.mtgpu_scan_headings_device(s._ctx, d_rec.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), 4, None, 0, None, k,
                                            1, min_objects, allow, out["flags"].data_ptr(), out["centres"].data_ptr(), out["blobs"].data_ptr(),
                                            out["objects"].data_ptr(), out["list"].data_ptr(), mot, out["allowed"].data_ptr(), None)
        torch.cuda.synchronize()
        return rc, lib.mtgpu_last_error().decode()

    good = out["motion"].data_ptr()
    for k, mo, allow, mot, word in ((4, 5, 255, good, "min_objects is 5, above k = 4"), (4, 1, 256, good, "allow 256"), (4, 1, -1, good, "allow -1"),
                                    (0, 1, 255, good, "k is 0"), (17, 1, 255, good, "k is 17"), (4, 1, 255, good + 8, "d_motion must be 16-byte aligned"),
                                    (4, 1, 255, host_motion.ctypes.data, "d_motion is not memory of device")):
        rc, msg = call(k, mo, allow, mot)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (word, msg)
        fresh, got = to_host(junk_outputs(4, 4)), to_host(out)
        for name in OUTPUTS:
            assert got[name].tobytes() == fresh[name].tobytes(), (word, name)
        assert (host_motion == JUNK).all()
    rc, msg = call(4, 4, 255, good)
    assert rc == _abi.MT_OK, msg
    assert_outputs(to_host(out), hi.hand_want(16, 4), "after the refusals", p, 4)


def test_contract_program_in_c(tmp_path):
    """tests/c/abi_headings_canaries.c: every refusal with the argument named and canary-filled outputs untouched; the
    caller-sized buffers exactly as the header sizes them, from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_headings_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_headings_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all heading buffers respected" in out.stdout


# ------------------------------------------------------------------ 9. example and command

def test_plain_c_headings_example(tmp_path):
    """examples/headings_example.c: a car going E and a walker going W in one frame, from plain C in a child process (it
    checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "headings_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "headings_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "object 0: 12 cells, heading E, 36 records, mean (+8.00, +0.00)" in out.stdout
    assert "object 1: 4 cells, heading W, 8 records, mean (-3.00, +0.00)" in out.stdout
    assert "against the traffic: 20 of 60 frames" in out.stdout


def test_end_to_end_command(gpu_scanner_factory, tmp_path, capsys):
    """A .mtmv of the sweep input's first stream with a third of its records pointing W, then `python -m
    mvtrim_amd.headings --json` in a fresh child process and the table form in this one."""
    p, mv, off, sd, pts, soff = oi.streams_case()
    F = oi.STREAM_FRAMES
    mv = mv.copy()
    rows = mv["dst_y"] >> 4
    west = (rows - 5) % 6 == 3                        # every second blob (rows 8, 14, ...) moves W
    mv["src_x"][west] = mv["dst_x"][west] + 5
    frames = [mv[int(off[f]):int(off[f + 1])] for f in range(F)]
    path = str(tmp_path / "stream.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    batch, fpts, hdr = tune.load(path)
    s = gpu_scanner_factory(p)
    mp = m.MergeParams(duration=F / 25.0, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    direct = headings.measure(s, batch, fpts, [1, 2, 4], mp, 1 << hi.W, 16, 2)
    want = hm.model_batch(p, mv, off[:F + 1], sd[:F], 16, 2, 1 << hi.W)
    per_frame = oi.stream_objects()[:F]
    assert [r["motion_frames"] for r in direct["levels_all"]] == [int((per_frame >= lv).sum()) for lv in (1, 2, 4)]
    assert [r["motion_frames"] for r in direct["levels_allow"]] == [int((want["allowed"] >= lv).sum()) for lv in (1, 2, 4)]
    assert direct["headings"]["E"] + direct["headings"]["W"] == int(per_frame.sum()) and direct["headings"]["W"] == int(want["allowed"].sum()) > 0
    assert direct["headings"]["none"] == 0 and direct["allow"] == "W"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [path, "--vectors-needed", "1", "--max-gap-sec", "0.1", "--padding-sec", "0.04", "--min-savings-pct", "5", "--min-blob-cells", "2"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.headings"] + args + ["--min-objects", "1,2,4", "--allow", "W", "--json"],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    for name in ("levels_all", "levels_allow", "headings", "allow", "records"):
        assert doc[name] == direct[name], name
    capsys.readouterr()
    assert headings.main(args + ["--ignore", "E", "--top", "3"]) == 0
    text = capsys.readouterr().out
    assert "headings allowed: all" in text and "headings allowed: SE,S,SW,W,NW,N,NE" in text and "object headings (top 3):" in text
    assert direction.names_from_allow(0xFF & ~1) == "SE,S,SW,W,NW,N,NE"
