"""CPU tier of tests/test_gpu_blob_edges.py: the models return every number the GPU tier states by hand, the inputs reach
what the GPU tests rely on (frame lengths on the loop bounds, the pan found where the still records are in the majority
and nowhere else among the test frames, squares on both sides of 2^32), the blob model's centres are the unchanged
oracle's on every batch used, and its labelling is scipy's where scipy imports."""
import numpy as np
import pytest

import blob_edges_inputs as bei
import blobs_model as bm
import derived_edge_inputs as dei
import derived_soak as dsoak
import gmc_blobs_inputs as gbi
import oracle_binding as ob
import zones_inputs as zi

COUNTS = ("centres", "blobs", "largest")
BLOB_KEYS = COUNTS + ("box",)


def same(a, b, keys=BLOB_KEYS):
    return all(np.asarray(a[k]).astype(np.int64).tolist() == np.asarray(b[k]).astype(np.int64).tolist() for k in keys)


def rows_of(r, f):
    return tuple(int(r[k][f]) for k in COUNTS) + (tuple(int(x) for x in r["box"][f]),)


# ------------------------------------------------------------------ a. head, step boundary and tail

def test_edge_batch_is_the_one_the_numbers_were_taken_on():
    mv, off, sd, test, cells, lengths = dei.edge_batch()
    assert (len(off) - 1, len(mv), len(test)) == (137, 443572, bei.N_TEST)
    long = bei.long_test_frames()
    short = [f for f in test if f not in long]
    assert (len(long), len(short)) == (bei.N_LONG, bei.N_SHORT)
    assert sorted({lengths[f][1] for f in short}) == list(range(7, 17))
    assert sum(lengths[f][1] >= 13 for f in short) < len(short)      # some short frames hold fewer than 13 voters
    # the first records of the test frames sit on all 16 residues of a 128-byte line, in both record sizes
    assert {int(off[f]) % 16 for f in long} == set(range(16))
    assert all(dei.head_of(off[f]) == lengths[f][0] for f in test)


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_edge_model_returns_the_hand_values(vn):
    """2 / 1 / 2 and the box of A + N on all 68 test frames at level 3, nothing at level 4, nothing on a filler frame; the
    all-ones-keep model in two streams is the unmasked one; the centres are the oracle's."""
    mv, off, sd, test, cells, _ = dei.edge_batch()
    p = bei.edge_params(vn)
    want, hand = bei.edge_model(vn), bei.edge_hand(vn)
    assert same(want, hand)
    assert same(bei.edge_model(vn, masked=True), want)
    assert want["centres"].tolist() == ob.scan_centres(p, mv, off, sd, nthreads=4)[1].tolist()
    assert want["centres"].tolist() == dei.edge_hand_sweep()[1, vn - 3].tolist()
    if vn == 3:
        assert rows_of(want, test[0]) == (2, 1, 2, (2, 5, 3, 5))
        assert int((want["centres"] > 0).sum()) == bei.N_TEST
        filler = [f for f in range(len(sd)) if f not in test]
        assert all(rows_of(want, f) == (0, 0, 0, bm.NO_BOX) for f in filler)
    else:
        assert not want["centres"].any() and (want["box"] == 0xFFFF).all()


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_compensated_model_at_max_shift_0_is_the_blob_model(vn):
    """Consequence A on the edge batch, without a keep and under all-ones keeps; info holds exact record counts: n_in is
    the number of records inside the bounds, n_x and n_y those of them that do not move on the axis."""
    mv, off, sd = dei.edge_batch()[:3]
    p = bei.edge_params(vn)
    plain = bei.edge_gmc_model(vn, False, 0)
    assert same(plain, bei.edge_model(vn)) and same(bei.edge_gmc_model(vn, False, 0, masked=True), plain, BLOB_KEYS + ("info",))
    assert not plain["info"][:, :4].any()
    ce, rows = dsoak.gmc_counts_np(p, mv, off, sd, 0, bei.Q8)
    assert ce.tolist() == plain["centres"].tolist() and rows.tolist() == plain["info"].tolist()
    assert int(plain["info"][:, 4].sum()) > 400000 and (plain["info"][:, 5] <= plain["info"][:, 4]).all()


@pytest.mark.parametrize("vn", bei.EDGE_VN)
def test_the_pan_is_found_on_the_long_frames_and_only_there(vn):
    """The pan-moved batch, (7, -3), max_shift 16, min_share_q8 128: found on exactly the 44 long test frames, where all
    five blob outputs are the plain model's on the original; the 24 short ones (7 .. 16 records, up to 13 of them
    voters) do not find it and read what the model says.  min_share_q8 0 changes nothing about which frames find it."""
    mv, off, sd, test, _, _ = dei.edge_batch()
    pmv, _, _ = bei.pan_batch()
    for k in ("src_x", "src_y"):
        assert pmv[k].dtype == np.int16
        assert np.array_equal(pmv[k].astype(np.int64) - mv[k], np.full(len(mv), -bei.PAN[0] if k == "src_x" else -bei.PAN[1]))
    assert np.array_equal(pmv["dst_x"], mv["dst_x"]) and np.array_equal(pmv["dst_y"], mv["dst_y"])
    p = bei.edge_params(vn)
    want, plain = bei.edge_gmc_model(vn, True, bei.MS), bei.edge_model(vn)
    found = [f for f in test if tuple(want["info"][f][:2]) == bei.PAN]
    long = bei.long_test_frames()
    assert found == long and len(found) == bei.N_LONG
    loose = gbi.model_batch(p, pmv, off, sd, bei.MS, 0)
    assert [f for f in test if tuple(loose["info"][f][:2]) == bei.PAN] == long
    assert same({k: v[long] for k, v in want.items()}, {k: v[long] for k, v in plain.items()})
    assert same({k: v[long] for k, v in want.items()}, bei.edge_hand(vn, long))
    assert same(bei.edge_gmc_model(vn, True, bei.MS, masked=True), want, BLOB_KEYS + ("info",))
    ce, rows = dsoak.gmc_counts_np(p, pmv, off, sd, bei.MS, bei.Q8)
    assert ce.tolist() == want["centres"].tolist() and rows.tolist() == want["info"].tolist()
    # a long frame: every counted record but the 13 voters (which move by (8, -1) and (9, -4)) carries the pan on both axes
    i = want["info"][long]
    assert (i[:, 4] > 3500).all() and (i[:, 5] == i[:, 4] - 13).all() and (i[:, 6] == i[:, 4] - 13).all()


# ------------------------------------------------------------------ c. the shifted base

def test_unaligned_batch_carries_centres_and_blobs():
    mv, off, sd = dei.unaligned_batch()
    p = bei.unaligned_params()
    plain = bei.unaligned_model()
    assert int((plain["centres"] > 0).sum()) > 20 and int(plain["blobs"].max()) > 1
    assert plain["centres"].tolist() == ob.scan_centres(p, mv, off, sd, nthreads=4)[1].tolist()
    ones = bei.unaligned_model(None, "ones")
    assert same(ones, plain)
    keeps = bei.unaligned_keeps("random")
    assert 0.8 < keeps.mean() < 0.9
    masked = bei.unaligned_model(None, "random")
    assert masked["centres"].tolist() == zi.oracle_batch(p, mv, off, sd, bei.UNALIGNED_SOFF, keeps)[1].tolist()
    assert masked["centres"].tolist() != plain["centres"].tolist()
    for ms in bei.UNALIGNED_SHIFT_SETTINGS:
        un, ma = bei.unaligned_model(ms), bei.unaligned_model(ms, "random")
        ce, rows = dsoak.gmc_counts_np(p, mv, off, sd, ms, bei.Q8)
        assert ce.tolist() == un["centres"].tolist() and rows.tolist() == un["info"].tolist()
        assert int((un["centres"] > 0).sum()) > 20 and int((ma["centres"] > 0).sum()) > 20
        some = un["info"][:, 4] > 20                                  # the masked estimate counts fewer records
        assert some.sum() > 20 and (ma["info"][some, 4] < un["info"][some, 4]).all() and (ma["info"][:, 4] <= un["info"][:, 4]).all()
        if ms == 0:
            assert same(un, plain) and same(ma, masked)


# ------------------------------------------------------------------ d. squares at and beyond 2^32

@pytest.mark.parametrize("thr", dei.BIG_ACTIVITY_THRESHOLDS)
def test_big_frames_by_hand_and_by_the_models(thr):
    mv, off, sd = dei.big_frames()
    seen = set()
    for vn in bei.BIG_VN:
        p = bei.big_params(thr, vn)
        hand = bei.big_hand(thr, vn)
        seen |= set(hand["centres"])
        plain = bm.model_batch(p, mv, off, sd)
        assert same(plain, hand)
        assert plain["centres"].tolist() == ob.scan_centres(p, mv, off, sd)[1].tolist()
        comp = gbi.model_batch(p, mv, off, sd, 0, bei.Q8)
        assert same(comp, hand) and not comp["info"][:, :4].any()
    assert thr > 8.5e9 or seen == {0, 1}


def test_residual_square_beyond_32_bits_under_a_pan():
    mv, off, sd = bei.pan_big_frames()
    p = bei.big_params(bei.PAN_BIG_THR, bei.PAN_BIG_VN)
    for ms in (bei.PAN_BIG_MS, 0):
        hand, info = bei.pan_big_hand(ms)
        got = gbi.model_batch(p, mv, off, sd, ms, bei.Q8)
        assert same(got, hand) and got["info"].tolist() == [list(r) for r in info], ms
        ce, rows = dsoak.gmc_counts_np(p, mv, off, sd, ms, bei.Q8)
        assert ce.tolist() == hand["centres"] and rows.tolist() == [list(r) for r in info]
    # the uncompensated scans see 65 535^2 < 2^32: nothing
    assert not bm.model_batch(p, mv, off, sd)["centres"].any() and not ob.scan_centres(p, mv, off, sd)[1].any()


# ------------------------------------------------------------------ the labelling

def test_model_labels_the_planes_of_these_batches_as_scipy_does():
    ndimage = pytest.importorskip("scipy.ndimage")
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    mv, off, _ = dei.unaligned_batch()
    p = bei.unaligned_params()
    keeps = bei.unaligned_keeps("random")
    planes = [bm.centre_plane(p, mv[int(off[f]):int(off[f + 1])], k) for f in range(len(off) - 1) for k in (None, keeps[int(f >= 13)])]
    emv, eoff = dei.edge_batch()[:2]
    planes += [bm.centre_plane(bei.edge_params(3), emv[int(eoff[f]):int(eoff[f + 1])]) for f in dei.edge_batch()[3][:8]]
    for cen in planes:
        lab, n = ndimage.label(cen, structure=four)
        mine = bm.label(cen)
        assert int(mine.max()) == n
        pairs = set(zip(lab[cen].tolist(), mine[cen].tolist()))
        assert len(pairs) == n and len({a for a, _ in pairs}) == n and len({b for _, b in pairs}) == n
        assert not mine[~cen].any()
