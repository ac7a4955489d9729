"""CPU tier: the pipe rounds of tests/pipe_soak.py — the inputs of tests/test_gpu_pipe_soak.py — without a GPU.  On the
default seed's first 60 iterations: the two sources of every expected value agree, a pipe form is supported where the
resident kernel's preview says so, and the rounds reach what they were built to reach (the counts are asserted, and
recorded in docs/rounds/r16_pipe_soak.md).  The hand shapes of the word-seam test are held against their models and,
masked, against the oracle on filtered records."""
import functools

import numpy as np
import pytest

import derived_soak as dsoak
import pipe_gmc_inputs as pgi
import pipe_soak as ps

REPLAYED = 60

# Measured on the first 60 draws of the default seed, from the models alone (47 of the 60 support every form):
MEASURED = dict(words2=43, margin=30, seam_split=14, growth=31, none_frames=48, vector_left_right=27, vector_masked=39, blob_flag_off=10)
# a floor of half the measured value, never below 5 of 60
FLOOR = {k: max(5, v // 2) for k, v in MEASURED.items()}


def forms_of(r, keeps):
    """(form, keep) of everything tests/test_gpu_pipe_soak.py compares on a round, where the grid supports it."""
    sup = r["support"]
    out = [("plain", None)]
    if sup["masked"]:
        out += [("masked", k) for k in keeps + ["ones"]]
    if sup["blobs"]:
        out += [("blobs", None)] + ([("blobs", r["blob_plane"])] if sup["masked"] else [])
    if sup["gmc"]:
        out += [("gmc", None)] + ([("gmc", k) for k in keeps + ["ones"]] if sup["masked"] else [])
    return out


@functools.lru_cache(maxsize=None)
def replayed():
    """[(d, r)] of the creatable draws among the first 60, every supported form's expected values with check_sources."""
    rng = np.random.RandomState(dsoak.DEFAULT_SEED)
    out = []
    for it in range(1, REPLAYED + 1):
        d = dsoak.draw(rng, it)
        if not d["creatable"]:
            continue
        r = ps.pipe_round(d)
        for form, keep in forms_of(r, [k for k in ("left", "right", "drawn") if k in r["planes"]]):
            ps.expected_pipe(d, r, form, keep, check_sources=True)
        out.append((d, r))
    return out


def test_sources_agree_and_all_ones_is_no_keep():
    for d, r in replayed():
        sup = r["support"]
        if sup["masked"]:
            assert ps.expected_pipe(d, r, "masked", "ones") == ps.expected_pipe(d, r, "plain"), d["it"]
        if sup["masked"] and sup["gmc"]:
            assert ps.expected_pipe(d, r, "gmc", "ones") == ps.expected_pipe(d, r, "gmc"), d["it"]
            if r["max_shift"] == 0:                              # no compensation: the masked scan on the same records
                for k in ("left", "right"):
                    e = ps.expected_pipe(d, r, "gmc", k)
                    assert not any(e["vector"])
                    assert pgi.masked_plain(r["params"], r["frames_gmc"], r["planes"][k]) == (e["flags"], e["centres"]), (d["it"], k)
        if sup["blobs"] and r["min_blob_cells"] <= 1:            # 0 and 1 change no flag
            assert ps.expected_pipe(d, r, "blobs")["flags"] == ps.expected_pipe(d, r, "plain")["flags"], d["it"]


def test_pipe_support_is_the_resident_previews():
    unsupported = 0
    for d, r in replayed():
        assert r["support"] == {"masked": d["support"]["zones"], "blobs": d["support"]["blobs"], "gmc": d["support"]["gmc"]}, d["it"]
        assert ("drawn" in r["planes"]) == r["support"]["masked"]
        unsupported += not all(r["support"].values())
    assert 0 < unsupported < len(replayed())                     # the refusal path is drawn too


def test_rounds_leave_the_draw_alone_and_replay():
    d, r = ps.replay(dsoak.DEFAULT_SEED, 5)
    d0, r0 = replayed()[4]
    assert d0["it"] == 5 and np.array_equal(d["mv"], d0["mv"]) and np.array_equal(r["pipe_mv"], r0["pipe_mv"])
    for k in ("max_frames", "max_records", "n_buffers", "zero_copy", "compact", "c", "blob_plane"):
        assert r[k] == r0[k], k
    assert r["mv"] is d["mv"] and r["pipe_mv"] is not d["mv"] and r["pipe_mv"] is not d["gmc_mv"]
    for k in ("dst_x", "dst_y"):
        assert np.array_equal(r["pipe_mv"][k], d["mv"][k])
    # the fourth state is none of the other three, and another seed draws another round of the same draw
    a = np.random.RandomState([dsoak.DEFAULT_SEED, 5, ps.PIPE_SALT]).randint(0, 2 ** 31, size=4).tolist()
    assert a != np.random.RandomState([dsoak.DEFAULT_SEED, 5, dsoak.BLOBS_SALT]).randint(0, 2 ** 31, size=4).tolist()
    assert a != np.random.RandomState([dsoak.DEFAULT_SEED, 5]).randint(0, 2 ** 31, size=4).tolist()
    picks = {(x["max_frames"], x["records_kind"], x["n_buffers"], x["c"]) for x in (ps.pipe_round(d, s) for s in range(8))}
    assert len(picks) > 3


def test_rounds_reach_what_they_were_built_for():
    got = {k: 0 for k in MEASURED}
    geometry = dict(max_frames=set(), kinds=set(), n_buffers=set(), zero_copy=set(), planes=set())
    for d, r in replayed():
        for k, v in ps.reach(d, r).items():
            got[k] += bool(v)
        F = r["F"]
        geometry["max_frames"].add({1: "1", 3: "3", 7: "7", F: "F", F + 5: "F+5"}[r["max_frames"]])
        geometry["kinds"].add(r["records_kind"])
        geometry["n_buffers"].add(r["n_buffers"])
        geometry["zero_copy"].add(r["zero_copy"])
        geometry["planes"].add(r["blob_plane"])
        # frames as the pipe can express them
        for f in range(F):
            assert (r["frames"][f] is None) == (r["sd"][f] == 0) == (r["frames_gmc"][f] is None)
            if r["frames"][f] is not None:
                assert len(r["frames"][f]) == int(r["off"][f + 1]) - int(r["off"][f])
        left, right = r["planes"]["left"], r["planes"]["right"]
        assert not (left & right).any() and (left | right).all() and left[:, :r["c"]].all() and 1 <= r["c"] <= max(1, d["params"].grid_w - 1)
    print("reach on the first", REPLAYED, "draws:", got, "floors:", FLOOR)
    for k, floor in FLOOR.items():
        assert got[k] >= floor, (k, got[k], floor)
    assert {"1", "3", "7", "F", "F+5"} <= geometry["max_frames"] and geometry["kinds"] == {"growth", "two-mean", "whole"}
    assert geometry["n_buffers"] == {1, 2, 3} and geometry["zero_copy"] == {False, True} and geometry["planes"] == {"left", "right", "drawn"}
    some_empty = sum(any(f is not None and len(f) == 0 for f in r["frames"]) for _, r in replayed())
    assert some_empty >= 5                                       # an empty frame WITH side data is fed as an empty array


@pytest.mark.parametrize("width", list(ps.SEAM_WIDTHS))
def test_seam_shapes_against_their_models(width):
    r = ps.seam_round(width)
    p, gw = r["params"], ps.SEAM_WIDTHS[width]
    assert all(r["support"].values()) and (gw + 63) // 64 == {63: 1, 64: 1, 65: 2, 128: 2, 129: 3}[gw]
    assert p.vertical_margin >= 2 and p.grid_h - 2 * p.vertical_margin == 13 and (p.vectors_needed & 0xFF) > 0
    assert all(200 <= len(f) <= 999 for f in r["frames"]) and r["c"] == (64 if gw > 64 else 32)
    keeps = [k for k in r["planes"] if k != "ones"]
    assert len(keeps) == 2 * (2 + (gw > 63) + (gw > 64) + 1)
    for form, keep in [("plain", None)] + [(f, k) for f in ("masked", "blobs", "gmc") for k in [None] + keeps + ["ones"] if (f, k) != ("masked", None)]:
        ps.expected_pipe(None, r, form, keep, check_sources=True)
    ex = lambda form, keep=None: ps.expected_pipe(None, r, form, keep)      # noqa: E731
    assert ex("masked", "ones") == ex("plain") and ex("gmc", "ones") == ex("gmc") and ex("blobs", "ones") == ex("blobs")
    # the planes decide the vector: pan A under "left", pan B under "right", on every frame; an analysed row less changes
    # the counts of the split planes
    assert ex("gmc", "left")["vector"] == [pgi.pack_vector(*a) for a in ps.SEAM_PANS_A]
    assert gw == 65 or ex("gmc", "right")["vector"] == [pgi.pack_vector(*b) for b in ps.SEAM_PANS_B]   # 65: 39 records, no clear mode
    for form in ("masked", "gmc"):
        for k in ("left", "right") if gw != 65 else ("left",):      # 65 columns: right of the split lies the last column alone
            assert sum(ex(form, k)["centres"]) > sum(ex(form, k + "-row")["centres"]) > 0, (form, k)
    single = [k for k in ("col63", "col64") if k in r["planes"] and ps.SEAM_WIDTHS[width] - 1 > int(k[3:])]
    for k in single:                                             # a kept column that is not the last one holds centres
        assert sum(ex("masked", k)["centres"]) > sum(ex("masked", k + "-row")["centres"]) > 0, k
    assert not any(ex("masked", "last")["centres"])              # the last column is never a centre ...
    assert any(ex("gmc", "last")["vector"])                      # ... and still decides the estimate
    assert any(a > b for a, b in zip(ex("blobs")["largest"], ex("blobs", "left-row")["largest"]))
    assert any(a and not b for a, b in zip(ex("blobs")["flags"], ex("blobs", "col63" if "col63" in r["planes"] else "last")["flags"]))
