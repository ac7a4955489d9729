"""CPU tier: the inputs of tests/test_gpu_derived_edges.py do what the GPU tests rely on.  Every value the GPU tests
expect by hand is checked here against the oracle (and the numpy model of the activity maps), and the plans of the
sweep and of the activity map reach the forms the inputs were built for — with host arithmetic alone."""
import numpy as np
import pytest

import mvtrim_amd as m

import derived_edge_inputs as dei
import oracle_binding as ob
import test_gpu_activity as act
import test_gpu_motion_scalar as ms
import test_gpu_sweep as sw
from golden_cases import id_of, load_hand_cases


def plan_of(p, n_thr, n_vec):
    pv = m.sweep_preview(p, n_thr, n_vec, dei.MI355X_LDS)
    return pv["passes"], pv["thresholds_per_pass"]


# ------------------------------------------------------------------ A

def test_pass_shape_table_reaches_every_pass_size():
    """Five tiles of 30 720 B fit 163 840 B next to the masks on 1080p, all eight of 13 760 B on 720p; the table's passes
    hold 1, 2, 3, 4, 5, 6, 7 and 8 thresholds: NT = 1, 2, 4 and 8, the last two padded and unpadded."""
    hd = m.ScanParams.from_config(1920, 1080)
    assert [plan_of(hd, t, 8) for t in range(1, 9)] == [(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 4), (2, 4)]
    assert dei.sweep_tile_bytes(hd) == (30720, 62)
    sizes, full = set(), 0
    for name, (w, h, thr, vec, plan) in dei.PASS_SHAPES.items():
        p = m.ScanParams.from_config(w, h)
        assert plan_of(p, len(thr), len(vec)) == plan, name
        passes, per = plan
        sizes |= {per, len(thr) - per * (passes - 1)}
        full += len(thr) == 8 and len(vec) == 8
        assert len(set(vec)) == len(vec) and min(vec) >= 1
        ints = [t for t in thr if t not in (0.0, dei.INF)]
        assert all(t in dei.THR8 for t in ints)
        if len(thr) > 2:
            assert thr != sorted(thr) and thr != sorted(thr, reverse=True), name       # out_t matters
    assert sizes == {1, 2, 3, 4, 5, 6, 7, 8} and full == 2
    p720 = m.ScanParams.from_config(1280, 720)
    assert (p720.grid_w, p720.grid_h) == (80, 45) and [plan_of(p720, t, 8) for t in (6, 7, 8)] == [(1, 6), (1, 7), (1, 8)]


@pytest.mark.parametrize("name", list(dei.PASS_SHAPES))
def test_pass_shape_oracle_blocks_tell_the_settings_apart(name):
    p, mv, off, sd, thr, vec, plan, want = dei.pass_shape_case(name)
    assert want.shape == (len(thr), len(vec), len(off) - 1) and 12 <= len(off) - 1 <= 16 and int(np.diff(off.astype(np.int64)).max()) <= 3000
    ints = [i for i, t in enumerate(thr) if t not in (0.0, dei.INF)]
    for a in ints:
        for b in ints:
            if a < b and thr[a] != thr[b]:
                assert not np.array_equal(want[a], want[b]), (name, thr[a], thr[b])
            if a < b and thr[a] == thr[b]:
                assert np.array_equal(want[a], want[b])
    for a in range(len(vec)):
        for b in range(a + 1, len(vec)):
            assert not np.array_equal(want[:, a], want[:, b]), (name, vec[a], vec[b])
    if dei.INF in thr:
        assert thr.count(10) == 2 and 0.0 in thr and min(vec) >= 1
        assert int(want[thr.index(dei.INF)].max()) == 0
        assert int(want[thr.index(0.0)].min(axis=0).max()) > 0 and not np.array_equal(want[thr.index(0.0)], want[thr.index(2)])
    assert int(want.max()) > 0


def test_pass_shape_oracle_blocks_are_the_oracles():
    """The memoised per-setting passes give what tests/test_gpu_sweep.py's oracle_sweep gives."""
    p, mv, off, sd, thr, vec, plan, want = dei.pass_shape_case("1080p-4+3-specials")
    assert np.array_equal(want, sw.oracle_sweep(1920, 1080, {}, mv, off, sd, thr, vec))


# ------------------------------------------------------------------ B

@pytest.mark.parametrize("name", list(dei.SEAM_GRIDS))
def test_seam_inputs_are_chunked_and_counted_by_hand(name):
    width, height, thr, ch_want = dei.SEAM_GRIDS[name]
    p, mv, off, sd, thr, vec, hand = dei.seam_case(name)
    assert p.vertical_margin == 0 and (p.grid_w, p.grid_h) == {"64x600": (64, 600), "4k": (240, 135)}[name]
    ch, R, single, pv = dei.sweep_chunk_rows(p, len(thr), len(vec))
    print(name, "plan", pv, "chunk_rows", ch, "of", R, "one chunk would take", single)
    assert R == p.grid_h and pv["thresholds_per_pass"] == 1 and pv["passes"] == len(thr)
    assert pv["lds_bytes"] < single and ch == ch_want < R                # the chunked path
    # every row boundary of the analysed range carries a vertical pair, each level separates some pairs
    pairs = dei.seam_pairs(p.grid_w, p.grid_h)
    assert sorted(y for fr in pairs for _, y, _, _ in fr) == list(range(p.grid_h - 1))
    for fr in pairs:
        for (x0, y0, _, _), (x1, y1, _, _) in zip(fr, fr[1:]):
            assert y1 == y0 + 2 and abs(x1 - x0) >= 2 and 1 <= x0 <= p.grid_w - 2 and 1 <= x1 <= p.grid_w - 2
    want = sw.oracle_sweep(width, height, dei.SEAM_KW, mv, off, sd, thr, vec)
    assert np.array_equal(want, hand), (want.tolist(), hand.tolist())
    assert len({hand[t, v].tobytes() for t in range(len(thr)) for v in range(8)}) == 8 * len(thr) and int(hand.min(axis=2).max()) > 0
    rows = dei.seam_row_pairs(p.grid_w, ch)
    assert {y for _, y, _, _ in rows} == {ch - 1, ch}
    if name == "4k":
        assert [x for x, y, _, _ in rows if y == ch - 1] == [63, 127, 191]


# ------------------------------------------------------------------ C

def test_big_magnitudes_by_exact_integers():
    assert len(dei.BIG_THRESHOLDS) == 10 and 4294967296.0 in dei.BIG_THRESHOLDS and max(dei.BIG_THRESHOLDS) == 8589672450.5
    assert sorted(dei.BIG_CALLS[0] + dei.BIG_CALLS[1]) == sorted(dei.BIG_THRESHOLDS)
    for call in dei.BIG_CALLS:
        assert len(call) == 5 and call != sorted(call) and call != sorted(call, reverse=True)
    p = m.ScanParams.from_config(32768, 32768, **dei.BIG_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (32, 32, 0)
    assert m.sweep_preview(p, 5, 2)["passes"] == 1 and m.activity_preview(p)["acc_bits"] in (16, 32)
    mv, off, sd = dei.big_frames()
    assert (mv["dst_x"].astype(np.int64) >> 10).reshape(5, 4).tolist() == [[31, 31, 30, 30]] * 5 and (mv["dst_y"] >> 10 == 31).all()
    dx = mv["dst_x"].astype(np.int64) - mv["src_x"].astype(np.int64)
    dy = mv["dst_y"].astype(np.int64) - mv["src_y"].astype(np.int64)
    mags = [int(a) * int(a) + int(b) * int(b) for a, b in zip(dx, dy)]
    assert mags == [v for da, db in dei.BIG_D for v in (da[0] ** 2 + da[1] ** 2, db[0] ** 2 + db[1] ** 2, dei.BIG_HELPER, dei.BIG_HELPER)]
    assert dei.BIG_HELPER == 8456505346 and min(mags) >= 4292739361 and sum(v >= 2 ** 32 for v in mags) == 16
    seen = set()
    for thr in dei.BIG_THRESHOLDS:
        want = sw.oracle_sweep(32768, 32768, dei.BIG_KW, mv, off, sd, [thr], [1, 2])
        hand = [dei.big_hand_count(thr, 1), dei.big_hand_count(thr, 2)]
        assert want[0].tolist() == hand, (thr, want[0].tolist(), hand)
        seen |= {tuple(hand[0]), tuple(hand[1])}
    assert len(seen) >= 5                                              # the thresholds and the levels separate the frames
    for thr in dei.BIG_ACTIVITY_THRESHOLDS:
        for vn in (1, 2):
            pa = m.ScanParams.from_config(32768, 32768, mv_threshold_sq=thr, vectors_needed=vn, **dei.BIG_KW)
            a, c, f, counts = act.model_maps(pa, mv, off, sd, [0, 5], 0)
            act.assert_oracle_identities(pa, mv, off, sd, [0, 5], 0, c, f, "model")
            assert counts.tolist() == dei.big_hand_count(thr, vn) and int(c.sum()) == sum(dei.big_hand_count(thr, vn))
            # the last column holds the pair: active iff >= vn of its two magnitudes pass
            assert int(a[0, 31, 31]) == sum(1 for pair in dei.BIG_D if sum(dei.big_passes(x * x + y * y, thr) for x, y in pair) >= vn)


# ------------------------------------------------------------------ D

def test_edge_batch_covers_heads_steps_and_tails():
    mv, off, sd, test, cells, lengths = dei.edge_batch()
    F = len(off) - 1
    o = off.astype(np.int64)
    assert len(test) == 68 and len(mv) == int(off[-1]) < 500_000 and 16_384 < int(np.diff(o).max()) <= 16_400
    assert len({int(o[f]) * 40 % 128 for f in test}) == 16 and len({int(o[f]) * 8 % 128 for f in test}) == 16
    kinds = set()
    for f in test:
        h, n = lengths[f]
        assert h == dei.head_of(o[f]) and n == int(o[f + 1] - o[f]) >= 7
        kinds.add(n - h)
    assert kinds == {-1, 0, 1} | set(dei.BIG_KINDS)
    assert {dei.STEP40 * k + d for k in (1, 2) for d in (-1, 0, 1)} | {dei.STEP8 + d for d in (-1, 0, 1, 2)} <= kinds
    # the three voters of A over the batch: every position named, in the head, at a step boundary and in the tail
    rel = set()
    for idx, f in enumerate(test):
        h, n = lengths[f]
        a, b = int(o[f]), int(o[f + 1])
        fr = mv[a:b]
        (ax, ay), (nx, ny) = cells[f]
        d2 = (fr["dst_x"].astype(np.int64) - fr["src_x"]) ** 2 + (fr["dst_y"].astype(np.int64) - fr["src_y"]) ** 2
        in_a = (fr["dst_x"] >> 4 == ax) & (fr["dst_y"] >> 4 == ay) & (d2 > 0)
        in_n = (fr["dst_x"] >> 4 == nx) & (fr["dst_y"] >> 4 == ny) & (d2 > 0)
        assert int(in_a.sum()) == 3 and int(in_n.sum()) == min(10, n - 3) >= 4 and int((d2 > 0).sum()) == 3 + min(10, n - 3)
        assert set(d2[d2 > 0].tolist()) == {5} and abs(ax - nx) + abs(ay - ny) == 1
        for q in np.flatnonzero(in_a):
            rel |= {("q", int(q)) if q < 1 else ("h", int(q) - h), ("n", int(q) - n)}
    for want in (("q", 0), ("h", -1), ("h", 0), ("h", 1023), ("h", 1024), ("h", 4095), ("h", 4096), ("h", 8191), ("h", 8192),
                 ("n", -2), ("n", -1)):
        assert want in rel, want
    fill = sorted(set(range(F)) - set(test))
    assert len(fill) == 69 and all(2 <= int(o[f + 1] - o[f]) <= 17 for f in fill) and all(f - 1 in fill and f + 1 in fill for f in test)
    for f in test:                                        # the record in front of a test frame and the one behind it vote into its cell A
        (ax, ay), _ = cells[f]
        for q in (int(o[f]) - 1, int(o[f + 1])):
            r = mv[q]
            assert (int(r["dst_x"]) >> 4, int(r["dst_y"]) >> 4) == (ax, ay)
            assert (int(r["dst_x"]) - int(r["src_x"])) ** 2 + (int(r["dst_y"]) - int(r["src_y"])) ** 2 == 5
    hand = dei.edge_hand_sweep()
    want = sw.oracle_sweep(1920, 1080, {}, mv, off, sd, dei.EDGE_THR, dei.EDGE_VEC)
    assert np.array_equal(want, hand)
    assert hand[0, 0, list(test)].tolist() == [2] * 68 and int(hand.sum()) == 2 * 2 * 68
    for vn in (3, 4):
        p = m.ScanParams.from_config(1920, 1080, mv_threshold_sq=4.0, vectors_needed=vn)
        ha, hc, hf, soff = dei.edge_hand_maps(vn)
        a, c, f, _ = act.model_maps(p, mv, off, sd, soff, 0)
        assert np.array_equal(a, ha) and np.array_equal(c, hc) and np.array_equal(f, hf) and int(hf.sum()) == F
        act.assert_oracle_identities(p, mv, off, sd, soff, 0, hc, hf, "hand maps")
        assert int(hc.sum()) == (2 * 68 if vn == 3 else 0) and int(ha.sum()) == (2 * 68 if vn == 3 else 68) and int(ha[0].sum()) > 0 and int(ha[1].sum()) > 0


# ------------------------------------------------------------------ E

def test_unaligned_batch_counts_something():
    mv, off, sd = dei.unaligned_batch()
    want = sw.oracle_sweep(1920, 1080, {}, mv, off, sd, [4, 16], [1, 2])
    assert len({want[t, v].tobytes() for t in range(2) for v in range(2)}) == 4 and len(set(want[1, 1].tolist())) >= 8
    imv, ioff = ms.integer_frames(np.random.RandomState(2), ms.SIZES)
    scores = ms.oracle_scores(imv, ioff)
    assert (scores == np.floor(scores)).all() and scores.max() < 2 ** 53 and (scores[np.array(ms.SIZES) > 2] > 0).all()


# ------------------------------------------------------------------ F

def test_accumulator_boundary_input():
    p = m.ScanParams.from_config(1920, 1080)
    plan = m.activity_preview(p, dei.MI355X_LDS)
    assert plan["acc_bits"] == 16 and plan["max_run"] == 65535
    mv, off, sd = dei.acc_batch()
    assert len(mv) == 280_000 and len(off) == dei.ACC_FRAMES + 1 == 70_001 and dei.ACC_SPLIT == plan["max_run"]
    assert mv[:4].tobytes() * 3 == mv[8:20].tobytes()
    _, centres = ob.scan_centres(ob.params_from_config(1920, 1080), mv[:256], off[:65], sd[:64])
    assert centres.tolist() == [2] * 64
    a, c, f, _ = act.model_maps(p, mv[:256], off[:65], sd[:64], [0, 64], 0)
    ha, hc, hf = dei.acc_hand([64])
    assert np.array_equal(a, ha) and np.array_equal(c, hc) and np.array_equal(f, hf)
    ha, hc, hf = dei.acc_hand([dei.ACC_SPLIT, dei.ACC_FRAMES - dei.ACC_SPLIT])
    assert hf.tolist() == [65535, 4465] and int(ha.sum()) == 2 * 70_000 == int(hc.sum()) and int(ha[0].max()) == 0xFFFF
    assert int(dei.acc_hand([dei.ACC_FRAMES])[0].max()) == 70_000 > 0xFFFF       # one step past the field


# ------------------------------------------------------------------ G

@pytest.mark.parametrize("name,kw,case", load_hand_cases()[1], ids=id_of)
def test_hand_cases_fit_the_derived_kernels(name, kw, case):
    p = m.ScanParams.from_config(**kw)
    assert (p.grid_w, p.grid_h) == (10, 10)
    assert m.sweep_preview(p, 3, 3)["passes"] == 1 and m.activity_preview(p)["acc_bits"] == 32
    mv, off, sd, hand = dei.hand_case_batch(case)
    thr, vec = dei.hand_case_settings(kw)
    rest = {k: v for k, v in kw.items() if k not in ("width", "height", "mv_threshold_sq", "vectors_needed")}
    want = sw.oracle_sweep(kw["width"], kw["height"], rest, mv, off, sd, thr, vec)
    assert int(want[1, 1, 0]) == hand
    a, c, f, counts = act.model_maps(p, mv, off, sd, [0, 1], 0)
    assert int(c.sum()) == hand and f.tolist() == [int(sd[0])]


def test_hand_cases_all_thirty_and_the_base_batch():
    g, cases = load_hand_cases()
    assert len(cases) == 30
    base, mv, off, sd, hand = dei.hand_base_batch()
    assert len(hand) >= 15 and len(mv) == int(off[-1]) and 0 in sd.tolist()
    _, centres = ob.scan_centres(ob.params_from_config(**base), mv, off, sd)
    assert centres.tolist() == hand
