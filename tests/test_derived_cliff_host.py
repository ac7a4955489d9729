"""CPU tier: the inputs of tests/test_gpu_derived_cliff.py and tests/test_gpu_derived_soak.py do what the GPU tests rely
on — with host arithmetic, the oracle and the numpy models alone.  The limit shapes really are the last ones their
kernels support, their batches carry centres, every value written out by hand equals the oracle's, and the two
independent sources of every expected value agree exactly; the soak's draws reach the kernels and carry centres too."""
import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_cliff_inputs as dci
import derived_soak as dsoak
import zones_inputs as zi
from activity_model import assert_oracle_identities, model_maps

LDS = dci.MI355X_LDS
CASES = [(k, n) for k in dci.KERNELS for n in dci.shapes(k)]


def test_pixel_coordinates_of_every_shape_stay_inside_int16():
    # pixel coordinates stay inside int16: block_shift 1 everywhere but on the sweep's two-column grids
    for k in dci.KERNELS:
        for name, (gw, gh, _) in dci.shapes(k).items():
            sh = dci.shift_of(gw, gh)
            assert (max(gw, gh) + 1) << sh <= 32768 and (sh == 1 or (k.startswith("sweep") and gw == 2)), (k, name)


@pytest.mark.parametrize("kernel,name", CASES)
def test_shape_is_the_last_one_that_fits(kernel, name):
    """The kernel's preview and plan_preview succeed; one more row (tall) or column (wide) is MT_ERR_UNSUPPORTED, and
    the LDS left over is less than what that row or column would add.  The sweep's lds_bytes includes a mask buffer that
    takes whatever room is left, so its need is stated with the three-row minimum the plan falls back to.  The plane scan's
    "staged" shapes are the last ones whose plane rows fit as well — one more is supported, unstaged, and a shape of its
    own — and its last shapes are the direction scan's; `staged` is asserted on each."""
    gw, gh, kind = dci.shapes(kernel)[name]
    p = dci.grid_params(gw, gh)
    pv = dci.kernel_preview(kernel, p)
    assert pv is not None and dci.creatable(p) and pv["lds_bytes"] <= LDS
    more = dci.one_more(gw, gh, dci.grows(name) if kernel == "lanes" else kind)
    p_more = dci.grid_params(*more)
    assert dci.creatable(p_more)                                     # the GPU test creates a context for it
    if kernel == "activity":
        assert pv["lds_bytes"] == dci.act_lds(gw, gh, pv["acc_bits"])
        i = dci.ACT_OUTCOMES.index((pv["acc_bits"], 2 * pv["lds_bytes"] <= LDS))
    if kernel == "lanes":
        # staged up to the "staged" shape, read from memory from the "unstaged" one on, up to the direction scan's limit
        staged = "-staged-" in name
        assert pv["staged"] == (1 if staged else 0) and pv["lds_bytes"] == dci.lanes_lds(gw, gh, staged)
        assert pv["plane_bytes"] == gw * gh
        if "-unstaged-" in name:
            before = (gw - 1, gh) if dci.grows(name) == "wide" else (gw, gh - 1)
            assert dci.kernel_preview(kernel, dci.grid_params(*before))["staged"] == 1
            return
        if staged:
            pm = dci.kernel_preview(kernel, p_more)
            assert pm is not None and pm["staged"] == 0 and more + ("plan",) in dci.shapes(kernel).values()
            used = dci.lanes_lds(gw, gh, True)
            assert 0 <= LDS - used < dci.lanes_lds(*more, True) - used
            return
        assert (gw, gh, kind) in dci.shapes("dir").values()          # the last unstaged grid is the direction scan's limit
    if kind == "plan":
        # not the last shape of the map, but the last (or, "past": the first) of its plan outcome
        bits, two = dci.ACT_OUTCOMES[i]
        if "past" in name:
            assert dci.act_outcome(gh - 1) == i - 1 and dci.act_outcome(gh) == i
            return
        assert dci.act_outcome(gh + 1) == i + 1
        limit = LDS // 2 if two else LDS
        used = dci.act_lds(gw, gh, bits)
        assert 0 <= limit - used < dci.act_lds(gw, gh + 1, bits) - used
        return
    assert dci.kernel_preview(kernel, p_more) is None
    need = dci.lds_need(kernel, gw, gh)
    if kernel.startswith("sweep"):
        n = 1 if kernel == "sweep1" else 8
        ch, R, _, spv = dci.sweep_chunk_rows(p, n, n)
        W = (gw + 63) // 64
        assert spv["thresholds_per_pass"] == 1 and need == spv["lds_bytes"] - n * (ch - 1) * W * 8
        assert LDS - spv["lds_bytes"] < n * W * 8 or ch == R          # the buffer took all the room a whole row fits in
    elif kernel in ("zones", "gmc", "dir", "lanes"):
        assert need == pv["lds_bytes"]
    else:
        assert pv["acc_bits"] == 0 and need == pv["lds_bytes"]
    added = dci.lds_need(kernel, *more) - need
    assert 0 <= LDS - need < added, (kernel, name, LDS - need, added)


def test_narrow_tall_zones_take_the_second_staging_trip():
    for name, (gw, gh, kind) in dci.shapes("zones").items():
        if name.startswith("tall") and gw in (2, 3, 65):
            assert gh * ((gw + 63) // 64) > dci.KEEP_TRIP, name
    gw, gh, _ = dci.shapes("zones")[[n for n in dci.shapes("zones") if n.startswith("tall-2x")][0]]
    assert gh > 4 * dci.KEEP_TRIP                                    # five keep words per lane


@pytest.mark.parametrize("gw", [3, 65])
def test_keep_words_of_the_second_staging_trip_decide_counts(gw):
    """What the masked scan would count if the keep words from word 1024 on never reached LDS, restated on the CPU: with
    zeros in their place the all-ones stream loses centres, with ones in their place the stream with 30 % of its cells
    cleared gains some — no constant serves both, so a kernel that drops the second trip cannot pass these shapes."""
    name = [n for n in dci.shapes("zones") if n.startswith(f"tall-{gw}x")][0]
    p, mv, off, sd, soff, keeps, _ = dci.zones_case(name)
    W = (gw + 63) // 64
    yy, xx = np.mgrid[0:p.grid_h, 0:gw]
    late = (yy * W + xx // 64) >= dci.KEEP_TRIP
    st = zi.stream_of_frames(soff, len(sd))
    want = zi.model_batch(p, mv, off, sd, soff, keeps)[0]
    for fill, stream in ((False, 0), (True, 1)):
        stale = keeps.copy()
        stale[:, late] = fill
        got = zi.model_batch(p, mv, off, sd, soff, stale)[0]
        assert (got != want)[st == stream].any(), (name, fill)


def test_sweep_8x8_shapes_take_several_passes_or_row_chunks():
    for name in dci.shapes("sweep8"):
        passes, ch, R = dci.sweep_path("sweep8", name)
        assert passes > 1 or ch < R, name
        assert passes == 8 and ch <= 3, name                         # one tile per pass, the three-row minimum or little more
    assert any(dci.sweep_path("sweep8", n)[1] < dci.sweep_path("sweep8", n)[2] for n in dci.shapes("sweep8"))


def test_activity_plan_outcomes_are_all_reached():
    seen = set()
    for name, (gw, gh, _) in dci.shapes("activity").items():
        pv = m.activity_preview(dci.grid_params(gw, gh))
        seen.add((pv["acc_bits"], 2 * pv["lds_bytes"] <= LDS))
    assert seen == set(dci.ACT_OUTCOMES)


def planted_is_planted(gw, gh, planted):
    """Corners, first / last row and column, both sides of a seam with horizontal and vertical pairs — wherever the grid
    has room for them."""
    cells = {c for pr in planted["E"] + (planted["H"] if gw <= 4 else []) for c in pr}
    assert {(0, 0), (gw - 1, 0), (0, gh - 1), (gw - 1, gh - 1)} <= cells
    if gw > 64:
        s = dci.seams_of(gw)
        assert len(s) == min(3, (gw - 1) // 64) or (gw - 1) // 64 <= 3
        for n in ("H",) + (("VL", "VR") if gh > 1 else ()):
            assert len(planted[n]) >= len(s), n
        assert all(a[1] == b[1] and a[0] % 64 == 63 and b[0] == a[0] + 1 for a, b in planted["H"])
        assert all(a[0] == b[0] and a[0] % 64 == 63 and b[1] == a[1] + 1 for a, b in planted["VL"])
        assert all(a[0] == b[0] and a[0] % 64 == 0 and b[1] == a[1] + 1 for a, b in planted["VR"])


def with_records(off):
    return np.diff(np.asarray(off).astype(np.int64)) > 0


@pytest.mark.parametrize("name", list(dci.shapes("zones")))
def test_zones_expected_values(name):
    p, mv, off, sd, soff, keeps, hand = dci.zones_case(name)
    gw, gh = p.grid_w, p.grid_h
    assert 6 <= len(sd) <= 12 and int((sd == 0).sum()) == 1 and int(((~with_records(off)) & (sd != 0)).sum()) >= 1
    planted_is_planted(gw, gh, dci.batch(gw, gh)[3])
    (fl, c, ca), (mc, mca) = dci.zones_expected(p, mv, off, sd, soff, keeps)
    assert np.array_equal(c, mc) and np.array_equal(ca, mca)
    assert np.array_equal(fl, (c >= 2).astype(np.uint8))
    for f, (hc, hca) in hand.items():
        assert (int(c[f]), int(ca[f])) == (hc, hca), (name, f)
    assert keeps[0].all() and 0.25 < 1.0 - keeps[1].mean() < 0.35
    if gw == 2:
        # no column in [1, gw - 2]: the reference counts no centre on such a grid, whatever the input
        assert not c.any() and not ca.any()
        return
    rec = with_records(off)
    assert 2 * int((c[rec] > 0).sum()) >= int(rec.sum())
    assert zi.counts_to_count(c, ca, off, sd)
    if gw > 64 and gh > 1:
        seam = [f for f in hand if zi.stream_of_frames(soff, len(sd))[f] == 2]
        # (a vertical pair in the grid's last column holds no centre with or without the mask: gw = 65)
        assert len(seam) == 3 and all(hand[f][0] == 0 for f in seam) and sum(hand[f][1] > 0 for f in seam) >= 2


@pytest.mark.parametrize("name", list(dci.shapes("activity")))
def test_activity_expected_values(name):
    p, mv, off, sd, soff, planted = dci.activity_case(name)
    gw, gh = p.grid_w, p.grid_h
    rec = with_records(off)
    for mc in (0, 1):
        want = model_maps(p, mv, off, sd, soff, mc)
        oc = assert_oracle_identities(p, mv, off, sd, soff, mc, want[1], want[2], "model")
        assert np.array_equal(oc[sd != 0], want[3][sd != 0]) and not want[3][sd == 0].any()   # whatever min_centres is
        assert gw == 2 and mc == 1 or (int(want[0].sum()) > 0 and int(want[2].min()) > 0)
    want0, want1 = model_maps(p, mv, off, sd, soff, 0), model_maps(p, mv, off, sd, soff, 1)
    if gw == 2:
        assert int(want0[1].sum()) == 0 and int(want1[2].sum()) == 0   # no centre can exist; min_centres 1 keeps no frame
    else:
        assert 2 * int((want0[3][rec] > 0).sum()) >= int(rec.sum())
        assert int(want1[2].sum()) < int(want0[2].sum())               # the empty frame with side data stays out
    # the planted frames alone: per-cell values by hand
    pmv, poff, psd, psoff, ha, hc, hf = dci.activity_planted_case(name)
    got = model_maps(p, pmv, poff, psd, psoff, 0)
    assert np.array_equal(got[0], ha) and np.array_equal(got[1], hc) and np.array_equal(got[2], hf)
    assert_oracle_identities(p, pmv, poff, psd, psoff, 0, hc, hf, "hand")
    assert int(ha[0, [0, -1]].sum()) > 0 and int(ha[0, :, [0, -1]].sum()) > 0 and int(hc[0, :, [0, -1]].sum()) == 0


@pytest.mark.parametrize("kernel,name", [(k, n) for k in ("sweep1", "sweep8") for n in dci.shapes(k)])
def test_sweep_expected_values(kernel, name):
    gw, gh, _ = dci.shapes(kernel)[name]
    mv, off, sd, planted = dci.batch(gw, gh)
    rec = with_records(off)
    vecs = set()
    for thr, vec in dci.sweep_calls(kernel):
        vecs |= set(vec)
        want, model = dci.sweep_expected(kernel, name, thr, vec, 0), dci.sweep_expected(kernel, name, thr, vec, 1)
        assert want.shape == (len(thr), len(vec), len(sd)) and np.array_equal(want, model)
        for f, h in dci.sweep_hand(kernel, name, thr, vec).items():
            assert np.array_equal(want[:, :, f], h), (kernel, name, f)
        if 0 in vec and gw >= 3:
            full = want[:, vec.index(0)]
            assert (full[:, sd != 0] == gh * (gw - 2)).all() and (full[:, sd == 0] == 0).all()
    assert {0, 255} <= vecs
    if kernel == "sweep8":
        assert len(set(dci.THR8)) < 8 and len(set(dci.VEC8)) < 8 and dci.THR8 != sorted(dci.THR8) and dci.VEC8 != sorted(dci.VEC8)
    thr, vec = dci.sweep_calls(kernel)[0]
    first = dci.sweep_expected(kernel, name, thr, vec, 0)[0, 0]      # threshold 16 or 25, level 2
    if gw == 2:
        assert not first.any()
    else:
        assert 2 * int((first[rec] > 0).sum()) >= int(rec.sum())


def test_gmc_shapes_are_the_ones_worked_by_hand():
    """16 (gh + 2) + 2080 <= 163 840 on two columns (tile and mask plane take eight bytes a row each); 20 (gh + 2) on
    three; (4 * 65 + 16) (gh + 2) and (4 * 193 + 32) (gh + 2), less the tile's padding, on 65 and 193."""
    tall = {gw: gh for gw, gh, kind in dci.shapes("gmc").values() if kind == "tall"}
    assert tall == {2: 10108, 3: 8086, 65: 584, 193: 199}
    assert len(dci.shapes("gmc")) == len(dci.shapes("zones")) == 6
    # a mask plane that starts on an odd number of 64-bit words is among them
    assert any(((gh + 2) * ((gw + 63) // 64)) % 2 for gw, gh, _ in dci.shapes("gmc").values())


@pytest.mark.parametrize("name", list(dci.shapes("gmc")))
def test_gmc_expected_values(name):
    """The numpy model and the oracle (consequence C) agree on the shape's batch under both settings; the planted pan
    frames have their hand values in the model and in the oracle."""
    import gmc_inputs as gi
    import gmc_model as gm
    import oracle_binding as ob
    gw, gh, _ = dci.shapes("gmc")[name]
    mv, off, sd, planted = dci.batch(gw, gh)
    planted_is_planted(gw, gh, planted)
    p = dci.grid_params(gw, gh, **dci.CTX_KW)
    for ms, q8 in dci.GMC_SETTINGS:
        fl, ce, rows = dci.gmc_expected(gw, gh, ms, q8)
        fits, oc = dci.gmc_oracle_c(gw, gh, rows)
        assert fits.all() and np.array_equal(oc, ce), (name, ms)      # every shifted src stays in int16 on these shapes
        assert np.array_equal(fl, (ce >= 2).astype(np.uint8)) and not ce[sd == 0].any() and not rows[sd == 0].any()
        if ms == 0:
            assert not rows[:, :4].any() and np.array_equal(ce, ob.scan_centres(p, mv, off, sd, nthreads=4)[1])
            assert gw == 2 or 2 * int((ce[with_records(off)] > 0).sum()) >= int(with_records(off).sum())
        else:                                                         # a blob frame's movers can be its mode: fewer centres
            assert gw == 2 or ce.any()
            print(name, "max_shift", ms, "centres", ce.tolist(), "applied", rows[:, :2].tolist())
    pp, pmv, poff, psd, hc, hi = dci.gmc_pan_case(name)
    fl, ce, info = gm.gmc_batch(pp, pmv, poff, psd, dci.GMC_PAN_MAX_SHIFT, 128)
    assert ce.tolist() == hc.tolist() and gi.info_rows(info).tolist() == hi.tolist(), name
    assert (2 * hi[:, 5] > hi[:, 4]).all()                            # the fillers outnumber the pair records
    moved = gm.shift_src(pmv, poff, hi[:, 0], hi[:, 1])
    assert ob.scan_centres(pp, moved, poff, psd)[1].tolist() == hc.tolist()
    plain = ob.scan_centres(pp, pmv, poff, psd)[1]
    assert gw == 2 or (hc[0] > 0 and (plain >= hc).all())             # without compensation every pair passes the threshold
    assert gm.gmc_batch(pp, pmv, poff, psd, 0, 128)[1].tolist() == plain.tolist()


# ------------------------------------------------------------------ the direction scan and the plane scan

def test_directed_batches_share_everything_but_the_pairs_displacements():
    """The directed planting changes src of the planted pairs' records and nothing else: the blob frames, N, Z, the
    permutations and the padding bytes are those of batch()."""
    for gw, gh, _ in dci.shapes("dir").values():
        a, b = dci.batch(gw, gh), dci.dir_batch(gw, gh)
        assert a[3] == b[3] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        for k in ("dst_x", "dst_y"):
            assert np.array_equal(a[0][k], b[0][k])
        fr = np.repeat(np.arange(len(dci.ORDER)), np.diff(a[1].astype(np.int64)))
        blob = ~np.isin(fr, [f for f, n in enumerate(dci.ORDER) if n in a[3]])
        assert np.array_equal(a[0].view(np.uint8).reshape(-1, 40)[blob], b[0].view(np.uint8).reshape(-1, 40)[blob])
        assert np.array_equal(a[0].view(np.uint8).reshape(-1, 40)[:, 34:], b[0].view(np.uint8).reshape(-1, 40)[:, 34:])
    sectors = {i % 8 for i in range(len(dci.dir_batch(65, dci.tallest("dir", 65))[3]["E"]))}
    assert sectors == set(range(8))                                   # E alone meets every sector


@pytest.mark.parametrize("name", list(dci.shapes("dir")))
def test_dir_expected_values(name):
    """The model under every byte of the chain and under the per-stream bytes equals the oracle on filtered records
    (consequence C); 0xFF the oracle on the records as they are; the planted frames have their hand values, and under
    0xFF those are hand_count's."""
    import dir_model as dm
    import oracle_binding as ob
    c = dci.dir_case(name)
    p, mv, off, sd, planted = c["params"], c["mv"], c["off"], c["sd"], c["planted"]
    gw, gh = p.grid_w, p.grid_h
    planted_is_planted(gw, gh, planted)
    assert {0x00, 0xFF} < set(dci.DIR_CHAIN) and len(set(dci.DIR_STREAM_ALLOWS)) == 3
    prev = None
    for allow in dci.DIR_CHAIN + (None,):
        fl, ce, rose = dci.dir_expected(name, allow)
        kw = dict(soff=c["soff"], allows=c["allows"]) if allow is None else dict(allow=allow)
        ofl, oce = dm.oracle_batch(p, mv, off, sd, **kw)
        assert np.array_equal(ce, oce) and np.array_equal(fl, ofl), (name, allow)
        for f, (hc, hr) in dci.dir_hand(c, allow).items():
            assert int(ce[f]) == hc and rose[f].tolist() == hr.tolist(), (name, allow, f)
        assert prev is None or np.array_equal(rose, prev)             # one rose whatever is allowed
        prev = rose
        assert rose.sum(axis=1).tolist() == dm.counting_moving(p, mv, off, sd).tolist()
    fl, ce, _ = dci.dir_expected(name, 0xFF)
    assert np.array_equal(ce, ob.scan_centres(p, mv, off, sd, nthreads=4)[1])
    for f, n in enumerate(dci.ORDER):
        if n in planted:
            assert dci.dir_hand(c, 0xFF)[f][0] == dci.hand_count(planted[n], gw, gh, 4.0, 2) == int(ce[f])
    if gw == 2:
        assert not ce.any()
        return
    e = dci.frames_named("E")[0]
    even, odd = (int(dci.dir_expected(name, a)[1][e]) for a in (0x55, 0xAA))
    assert even > 0 and odd > 0 and even + odd == int(ce[e]) and int(dci.dir_expected(name, 0x00)[1][e]) == 0


def corner_cells(gw, gh, margin=0):
    """The first and the last cell of the first and the last analysed row."""
    return [(0, margin), (gw - 1, margin), (0, gh - 1 - margin), (gw - 1, gh - 1 - margin)]


@pytest.mark.parametrize("name", list(dci.shapes("lanes")))
def test_lanes_expected_values(name):
    """Every rotation of the three planes over the three streams: the model equals the oracle on filtered records
    (consequence C), P_all alone the oracle on the records as they are, the planted frames have their hand values.  The
    flow maps: per stream and per frame against the hand maps, and their sums are the roses' (G).  The corners of the
    analysed rows hold bytes of their own, and a plane that loses its last one, two or three bytes, or arrives one byte
    late, changes a planted frame's count — what a short or shifted staged copy would do."""
    import lanes_model as lm
    import oracle_binding as ob
    c = dci.lanes_case(name)
    p, mv, off, sd, planted = c["params"], c["mv"], c["off"], c["sd"], c["planted"]
    gw, gh = p.grid_w, p.grid_h
    assert "E" in c["whole"] and m.lanes_preview(p)["staged"] == (1 if "-staged-" in name else 0)
    plain = ob.scan_centres(p, mv, off, sd, nthreads=4)[1]
    assert np.array_equal(lm.model_batch(p, mv, off, sd, c["planes"]["all"])[1], plain)
    st = zi.stream_of_frames(c["soff"], len(sd))
    for rot in dci.LANES_ROTATIONS:
        fl, ce, rose = dci.lanes_expected(name, rot)
        ofl, oce = lm.oracle_batch(p, mv, off, sd, dci.lanes_stack(c, rot), c["soff"])
        assert np.array_equal(ce, oce) and np.array_equal(fl, ofl), (name, rot)
        under_all = np.array([rot[s] == "all" for s in st])
        assert np.array_equal(ce[under_all], plain[under_all])
        for f, (hc, hr) in dci.lanes_hand(c, rot).items():
            assert (hc is None or int(ce[f]) == hc) and rose[f].tolist() == hr.tolist(), (name, rot, f)
    hands = [h[0] for rot in dci.LANES_ROTATIONS for h in dci.lanes_hand(c, rot).values()]
    assert hands.count(None) < len(hands) // 2 and (gw == 2 or (0 in hands and max(x or 0 for x in hands) > 0))
    # the flow maps
    each = dci.flow_expected(name, dci.FLOW_EACH)
    for f, n in enumerate(dci.ORDER):
        if n in planted:
            assert np.array_equal(each[f], dci.hand_flow(planted[n], gw, gh)), (name, f)
    assert not each[dci.frames_named("N")[0]].any() and not each[dci.frames_named("Z")[0]].any()
    per_stream = dci.flow_expected(name, dci.ZONE_SOFF)
    rose = dci.lanes_expected(name, dci.LANES_ROTATIONS[0])[2]
    for s in range(3):
        a, b = dci.ZONE_SOFF[s], dci.ZONE_SOFF[s + 1]
        assert np.array_equal(per_stream[s], each[a:b].sum(axis=0))
        assert per_stream[s].sum(axis=(1, 2)).tolist() == rose[a:b].sum(axis=0, dtype=np.uint64).tolist()
    if gw == 2:
        return                                                        # no column can hold a centre: the planes decide no count
    own = c["planes"]["own"]
    corners = [int(own[y, x]) for x, y in corner_cells(gw, gh)]
    # (on three columns the right corners are pairs 0 and 1 of H: the bytes of pairs 0 and 1 of E)
    assert all(corners) and (gh == 1 or len(set(corners)) >= (3 if gw > 4 else 2)), (name, corners)
    # the control: what a staged copy that drops tail bytes, or starts one byte late, would hand the vote
    frames = dci.frames_named("E") + dci.frames_named("H")
    for kind, want_rot in (("own", dci.LANES_ROTATIONS[2]), ("all", dci.LANES_ROTATIONS[1])):
        s = want_rot.index(kind)
        mine = [f for f in frames if st[f] == s]
        want = dci.lanes_expected(name, want_rot)[1]
        for cut in (1, 2, 3) if gw > 4 else (3,):                     # (three columns: the last column's pair holds no centre)
            short = c["planes"][kind].copy().reshape(-1)
            short[-cut:] = 0
            got = lm.model_batch(p, mv, off, sd, np.stack([short.reshape(gh, gw)] * 3), c["soff"])[1]
            assert any(got[f] != want[f] for f in mine), (name, kind, cut)
    late = np.roll(own.reshape(-1), 1).reshape(gh, gw)
    s = dci.LANES_ROTATIONS[2].index("own")
    got = lm.model_batch(p, mv, off, sd, np.stack([late] * 3), c["soff"])[1]
    want = dci.lanes_expected(name, dci.LANES_ROTATIONS[2])[1]
    assert any(got[f] != want[f] for f in frames if st[f] == s), name


def test_plane_base_phases_cover_every_combination():
    """Over the runs of test_lanes_plane_base_phases the source's phase inside a 32-bit word and the number of copied
    bytes modulo 4 take all sixteen combinations; every run but tall-65 of the unstaged limit is staged; the variant with
    a margin keeps the planted pairs on its analysed rows, where a plane whose rows are taken from gy - (y_lo - 1) in
    place of gy - y_lo — one row late — changes a planted frame's count."""
    import lanes_model as lm
    seen = set()
    for name, margin in dci.phase_runs():
        gw, gh, kind = dci.shapes("lanes")[name]
        c = dci.lanes_case(name, margin)
        assert m.lanes_preview(c["params"])["staged"] == (0 if kind == "tall" else 1) and c["params"].vertical_margin == margin
        if kind != "tall":
            seen |= dci.phase_pairs(gw, gh, margin)
    assert seen == {(a, b) for a in range(4) for b in range(4)}
    assert sum(1 for _, mg in dci.phase_runs() if mg) == 1 and len(dci.phase_runs()) == 8
    name, margin = [r for r in dci.phase_runs() if r[1]][0]
    c = dci.lanes_case(name, margin)
    p, gw, gh = c["params"], c["params"].grid_w, c["params"].grid_h
    own = c["planes"]["own"]
    assert all(int(own[y, x]) for x, y in corner_cells(gw, gh, margin)) and not own[:margin].any() and not own[gh - margin:].any()
    rot = dci.LANES_ROTATIONS[2]
    want = dci.lanes_expected(name, rot, margin)
    for f, (hc, hr) in dci.lanes_hand(c, rot).items():
        assert (hc is None or int(want[1][f]) == hc) and want[2][f].tolist() == hr.tolist()
    row_late = np.roll(own, -1, axis=0)                               # the byte of row gy + 1 where row gy's is wanted
    got = lm.model_batch(p, c["mv"], c["off"], c["sd"], np.stack([row_late] * 3), c["soff"])[1]
    e = dci.frames_named("E")[0]
    assert int(want[1][e]) > 0 and got[e] != want[1][e]


# ------------------------------------------------------------------ the soak's draws

SOAK_REPLAYED = 40


def test_soak_draws_reach_the_kernels_and_carry_centres():
    """The default seed's first 40 iterations: each kernel is supported in at least three quarters of them, at least half
    of the supported ones have a non-zero centre total, and the two sources of every expected value agree."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    supported = {k: 0 for k in dsoak.KERNELS}
    nonzero = {k: 0 for k in dsoak.KERNELS}
    for it in range(1, SOAK_REPLAYED + 1):
        d = dsoak.draw(rng, it)
        if it in (1, 7, SOAK_REPLAYED):
            again = dsoak.replay(dsoak.DEFAULT_SEED, it)
            assert again["params"] == d["params"] and np.array_equal(again["mv"], d["mv"]) and again["support"] == d["support"]
        for k in dsoak.KERNELS:
            if not d["support"][k]:
                continue
            supported[k] += 1
            nonzero[k] += dsoak.expected(d, k, check_sources=True)["total"] > 0
    for k in dsoak.KERNELS:
        assert 4 * supported[k] >= 3 * SOAK_REPLAYED, (k, supported)
        assert 2 * nonzero[k] >= supported[k], (k, nonzero, supported)
    assert min(supported.values()) < SOAK_REPLAYED                   # the unsupported answer is drawn too


# sha256 (first 16 hex digits) over mv, off, thr, vec and keeps of the default seed's first eight draws, as draw() made
# them before the compensated scan joined the soak
DRAWS_BEFORE_GMC = ["675b176ee95000a1", "182bcdb169c4ea7b", "9adf7a58e431347b", "4aa1079ab9b30ab6", "5846d0fb9f3d8f54",
                    "8ed9b9450ac5b6ea", "6ad47eaf9a24b42f", "23ad4b31b8bf6116"]


def draw_digest(d):
    import hashlib
    h = hashlib.sha256()
    for k in ("mv", "off", "thr", "vec", "keeps"):
        v = d.get(k)
        h.update(v.tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()[:16]


def test_soak_draws_are_what_they_were_before_the_compensated_scan_joined():
    """replay() and the recorded figures of docs/rounds/r07_derived_limits.md depend on the stream: the compensated scan's
    inputs come from a RandomState of their own, and its copy of the records leaves d["mv"] alone."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    for it, want in enumerate(DRAWS_BEFORE_GMC, start=1):
        d = dsoak.draw(rng, it)
        assert draw_digest(d) == want, it
        if d["creatable"] and len(d["mv"]) and d["gmc_follow"] > 0:
            assert d["gmc_mv"] is not d["mv"] and not np.array_equal(d["gmc_mv"], d["mv"])
            for k in ("dst_x", "dst_y"):
                assert np.array_equal(d["gmc_mv"][k], d["mv"][k])
    # another seed draws other pans for the same iteration, and the same seed the same ones
    a, b = dsoak.replay(dsoak.DEFAULT_SEED, 4), dsoak.replay(dsoak.DEFAULT_SEED, 4)
    assert np.array_equal(a["gmc_pans"], b["gmc_pans"]) and np.array_equal(a["gmc_mv"], b["gmc_mv"])
    c = dsoak.draw_gmc(dsoak.DEFAULT_SEED + 1, 4, a["params"], a["mv"], a["off"])
    assert not np.array_equal(a["gmc_pans"], c["gmc_pans"])


GMC_REPLAYED = 60


def test_soak_draws_reach_the_compensated_scan():
    """The default seed's first 60 iterations, from the reference alone: the compensated scan is supported in at least
    three quarters of the creatable draws; in at least a third of the supported ones some frame is compensated on some
    axis, in at least a third a compensated frame still has centres, and at least once a mode is found and not applied.
    (test_soak_draws_reach_the_kernels_and_carry_centres holds the two sources against each other on the first 40.)"""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    creatable = supported = compensated = with_centres = lost = 0
    shifts, shares, outside = set(), set(), 0
    for it in range(1, GMC_REPLAYED + 1):
        d = dsoak.draw(rng, it)
        creatable += d["creatable"]
        if not d["support"].get("gmc"):
            continue
        supported += 1
        e = dsoak.expected(d, "gmc")
        compensated += e["compensated"] > 0
        with_centres += e["compensated_with_centres"] > 0
        lost += e["found_not_applied"] > 0
        shifts.add(d["gmc_max_shift"])
        shares.add(d["gmc_share_q8"])
        outside += bool((np.abs(d["gmc_pans"]) > d["gmc_max_shift"]).any())
        assert (np.abs(d["gmc_pans"]) <= d["gmc_max_shift"] + 2).all()
    print("creatable", creatable, "supported", supported, "compensated", compensated, "with centres", with_centres, "found, not applied", lost)
    assert 4 * supported >= 3 * creatable and supported < creatable
    assert 3 * compensated >= supported and 3 * with_centres >= supported and lost >= 1
    assert shifts == set(dsoak.GMC_SHIFT_POOL) and shares == set(dsoak.GMC_SHARE_Q8_POOL) and outside >= 5


# sha256 (first 16 hex digits) over mv, off, thr, vec, keeps and the compensated scan's max_shift, min_share_q8, pans, follow
# share and records of the default seed's first eight draws, as draw() made them before the blob scans joined the soak
DRAWS_BEFORE_BLOBS = ["c4072ee87b7db2d0", "1132c46077c7206c", "9ec73fe13afb5ee1", "4332b96d77677b17", "d65343551ffc13e1",
                      "e6fb2e9100bf5bc2", "48c3bff0fbff536b", "1ad07dc68d9add95"]
GMC_FIELDS = ("gmc_max_shift", "gmc_share_q8", "gmc_pans", "gmc_follow", "gmc_mv")


def draw_digest_with_gmc(d):
    import hashlib
    h = hashlib.sha256(draw_digest(d).encode())
    for k in GMC_FIELDS:
        v = d.get(k)
        if isinstance(v, np.ndarray) and v.dtype.names:              # field by field: a copy of padded records need not
            for name in v.dtype.names:                               # carry the padding bytes over
                h.update(np.ascontiguousarray(v[name]).tobytes())
        else:
            h.update(v.tobytes() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()[:16]


def test_soak_draws_are_what_they_were_before_the_blob_scans_joined():
    """min_blob_cells and the mask decision come from a RandomState of their own, seeded apart from draw_gmc's: `rng`, the
    compensated scan's settings and its copy of the records are what they were."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    for it, want in enumerate(DRAWS_BEFORE_BLOBS, start=1):
        d = dsoak.draw(rng, it)
        assert draw_digest_with_gmc(d) == want, it
    a, b = dsoak.replay(dsoak.DEFAULT_SEED, 5), dsoak.replay(dsoak.DEFAULT_SEED, 5)
    assert (a["min_blob_cells"], a["blob_masked"]) == (b["min_blob_cells"], b["blob_masked"])
    picks = {(x["min_blob_cells"], x["blob_masked"]) for x in (dsoak.draw_blobs(s, 5, a["params"]) for s in range(12))}
    assert len(picks) > 3                                            # other seeds draw other settings for the same iteration
    # the third state is not draw_gmc's: the same (seed, it) gives another stream
    g = np.random.RandomState([dsoak.DEFAULT_SEED, 5]).randint(0, 2 ** 31, size=4)
    t = np.random.RandomState([dsoak.DEFAULT_SEED, 5, dsoak.BLOBS_SALT]).randint(0, 2 ** 31, size=4)
    assert g.tolist() != t.tolist()


BLOBS_REPLAYED = 60


def test_soak_draws_reach_the_blob_scans():
    """The default seed's first 60 iterations, from the models alone.  Measured: 60 creatable, each blob kernel supported
    in 47 of them; see the figures printed below and docs/rounds/r15_blob_edges.md."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    creatable = 0
    n = {k: dict(supported=0, multi=0, flag_off=0, flag_kept=0, masked=0, behind=0, vn0=0) for k in ("blobs", "gmc_blobs")}
    pool = set()
    for it in range(1, BLOBS_REPLAYED + 1):
        d = dsoak.draw(rng, it)
        creatable += d["creatable"]
        for k in n:
            if not d["support"].get(k):
                continue
            e = dsoak.expected(d, k)
            n[k]["supported"] += 1
            pool.add(d["min_blob_cells"])
            vn0 = (d["params"].vectors_needed & 0xFF) == 0
            n[k]["vn0"] += vn0
            if vn0 and k == "blobs" and not e["masked"]:              # one blob spanning the plane's inner columns
                p = d["params"]
                rows, has = max(0, p.grid_h - 2 * p.vertical_margin), zi.has_side_data(d["off"], d["sd"])
                assert (e["blobs"][has] == (1 if rows and p.grid_w > 2 else 0)).all() and (e["largest"][has] == rows * max(0, p.grid_w - 2)).all()
            for c in ("multi", "flag_off", "flag_kept", "behind"):
                n[k][c] += e[c] > 0
            n[k]["masked"] += e["masked"]
    print("creatable", creatable, n, "min_blob_cells seen", sorted(pool))
    for k, c in n.items():
        assert 4 * c["supported"] >= 3 * creatable and c["supported"] < creatable, (k, c)
        assert c["multi"] >= 1 and c["flag_off"] >= 1 and c["flag_kept"] >= 1, (k, c)
        assert 1 <= c["masked"] < c["supported"] and c["behind"] >= 1 and c["vn0"] >= 1, (k, c)
    assert {0, 1} <= pool and max(pool) >= 40


# sha256 (first 16 hex digits) over draw_digest_with_gmc and the blob scans' min_blob_cells and mask decision of the default
# seed's first eight draws, as draw() made them before the direction scan, the plane scan and the flow map joined the soak
DRAWS_BEFORE_DIR = ["86b018d452f6ec74", "c4252deebcbf5bf6", "17f93285a47ae65e", "73b424478bc157f9", "ea20f336fcf7fdb5",
                    "1c67ddf09c4c5e04", "f1b10d3462f80db8", "6c42a8f906a8a7b3"]


def draw_digest_with_blobs(d):
    import hashlib
    h = hashlib.sha256(draw_digest_with_gmc(d).encode())
    for k in ("min_blob_cells", "blob_masked"):
        h.update(repr(d.get(k)).encode())
    return h.hexdigest()[:16]


def test_soak_draws_are_what_they_were_before_the_direction_scans_joined():
    """The allow bytes, the planes and the forms of the calls come from a RandomState of their own, seeded apart from
    draw_gmc's and draw_blobs': `rng`, the compensated scan's inputs and the blob scans' settings are what they were."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    for it, want in enumerate(DRAWS_BEFORE_DIR, start=1):
        d = dsoak.draw(rng, it)
        assert draw_digest_with_blobs(d) == want, it
    a, b = dsoak.replay(dsoak.DEFAULT_SEED, 5), dsoak.replay(dsoak.DEFAULT_SEED, 5)
    assert (a["allow"], a["dir_per_stream"], a["lanes_one_plane"], a["plane_kinds"]) == (b["allow"], b["dir_per_stream"], b["lanes_one_plane"], b["plane_kinds"])
    assert np.array_equal(a["allows"], b["allows"]) and np.array_equal(a["planes"], b["planes"])
    S = len(a["zsoff"]) - 1
    assert a["allows"].shape == (S,) and a["planes"].shape == (S, a["params"].grid_h, a["params"].grid_w) and a["planes"].dtype == np.uint8
    picks = {(x["allow"], x["dir_per_stream"], x["lanes_one_plane"]) for x in (dsoak.draw_dir(s, 5, a["params"], S) for s in range(12))}
    assert len(picks) > 3                                            # other seeds draw other settings for the same iteration
    # the fourth state is neither draw_gmc's nor draw_blobs'
    streams = [np.random.RandomState([dsoak.DEFAULT_SEED, 5] + salt).randint(0, 2 ** 31, size=4).tolist()
               for salt in ([], [dsoak.BLOBS_SALT], [dsoak.DIR_SALT])]
    assert len({tuple(x) for x in streams}) == 3


DIR_REPLAYED = 60


def test_soak_draws_reach_the_direction_scans():
    """The default seed's first 60 iterations, from the models alone.  Each of the direction scan, the plane scan and the
    flow map is supported in at least three quarters of the creatable draws; in at least a third of the supported draws
    the drawn byte or plane turns off a flag the plain scan sets; the scalar and the per-stream form of the direction
    call, and the one-plane and the per-stream form of the plane call, all occur.  Measured: 60 creatable, 47 supported,
    a flag turned off in 22 (bytes) and 16 (planes), 23 and 33 per-stream calls, one unstaged plane call — which is
    reported and not asserted: tests/test_gpu_derived_cliff.py carries that form."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    creatable = 0
    n = {k: dict(supported=0, flag_off=0, per_stream=0, behind=0, vn0=0) for k in ("dir", "lanes")}
    flow = dict(supported=0, nonzero=0)
    unstaged, bytes_seen, kinds_seen = 0, set(), set()
    for it in range(1, DIR_REPLAYED + 1):
        d = dsoak.draw(rng, it)
        creatable += d["creatable"]
        for k in n:
            if not d["support"].get(k):
                continue
            e = dsoak.expected(d, k)
            n[k]["supported"] += 1
            n[k]["vn0"] += (d["params"].vectors_needed & 0xFF) == 0
            for c in ("flag_off", "behind"):
                n[k][c] += e[c] > 0
            n[k]["per_stream"] += e["per_stream"]
        if d["support"].get("dir"):
            bytes_seen |= {d["allow"]} | set(d["allows"].tolist())
        if d["support"].get("lanes"):
            unstaged += d["lanes_staged"] == 0
            kinds_seen |= set(d["plane_kinds"])
        if d["support"].get("flow"):
            flow["supported"] += 1
            flow["nonzero"] += dsoak.expected(d, "flow")["total"] > 0
    print("creatable", creatable, n, "flow", flow, "unstaged plane calls", unstaged, "bytes seen", sorted(bytes_seen))
    for k, c in n.items():
        assert 4 * c["supported"] >= 3 * creatable and c["supported"] < creatable, (k, c)
        assert 3 * c["flag_off"] >= c["supported"], (k, c)
        assert 1 <= c["per_stream"] < c["supported"] and c["behind"] >= 1 and c["vn0"] >= 1, (k, c)
    assert 4 * flow["supported"] >= 3 * creatable and 2 * flow["nonzero"] >= flow["supported"]
    assert {0x00, 0xFF} <= bytes_seen and kinds_seen == set(dsoak.PLANE_KINDS)


def test_soak_preview_says_unsupported_as_the_library_does():
    p = m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2)
    assert dsoak.support_of(p, 3, 3) == {"sweep": False, "activity": False, "zones": False}
    with pytest.raises(m.MtgpuError) as ei:
        m.zones_preview(p)
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
