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
    takes whatever room is left, so its need is stated with the three-row minimum the plan falls back to."""
    gw, gh, kind = dci.shapes(kernel)[name]
    p = dci.grid_params(gw, gh)
    pv = dci.kernel_preview(kernel, p)
    assert pv is not None and dci.creatable(p) and pv["lds_bytes"] <= LDS
    more = dci.one_more(gw, gh, kind)
    p_more = dci.grid_params(*more)
    assert dci.creatable(p_more)                                     # the GPU test creates a context for it
    if kernel == "activity":
        assert pv["lds_bytes"] == dci.act_lds(gw, gh, pv["acc_bits"])
        i = dci.ACT_OUTCOMES.index((pv["acc_bits"], 2 * pv["lds_bytes"] <= LDS))
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
    elif kernel in ("zones", "gmc"):
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


def test_soak_preview_says_unsupported_as_the_library_does():
    p = m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2)
    assert dsoak.support_of(p, 3, 3) == {"sweep": False, "activity": False, "zones": False}
    with pytest.raises(m.MtgpuError) as ei:
        m.zones_preview(p)
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
