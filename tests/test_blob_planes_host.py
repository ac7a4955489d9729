"""CPU tier of the random and adversarial centre planes (tests/blob_planes.py) that tests/test_gpu_blob_planes.py holds the
three labelling kernels to: the generators are deterministic and read-only, the flood-fill model labels every plane of
every batch as scipy does, every family reaches the regime it exists for on the committed seeds — no plane is left out
to make that so — both previews accept every grid and the pan embedding exists for every batch."""
import numpy as np
import pytest

import mvtrim_amd as m

import blob_planes as bp
import blobs_inputs as bi
import blobs_model as bm
import zones_inputs as zi

ALL_FAMILIES = list(bp.PERC) + ["maze", "comb_up", "comb_down", "bars", "confetti"]


def centre_planes(name):
    """(plane name or None, frame, centre plane) of every frame with side data of a batch, under its stream's keep."""
    b = bp.batch(name)
    F = len(b.sd)
    st = zi.stream_of_frames(b.soff, F) if b.keeps is not None else None
    by_frame = {f: n for n, f in b.frame_of.items()}
    per_stream = F // 2 if b.keeps is not None else F
    for f in range(F):
        if b.sd[f]:
            keep = None if b.keeps is None else b.keeps[st[f]]
            yield by_frame.get(f % per_stream), f, bm.centre_plane(b.p, b.mv[int(b.off[f]):int(b.off[f + 1])], keep)


# ------------------------------------------------------------------ the generators and the table

@pytest.mark.parametrize("family", ALL_FAMILIES)
def test_generators_are_deterministic_and_read_only(family):
    for gw, rows, seed in ((63, 12, 3), (65, 34, 4), (130, 21, 5)):
        a, b = bp.plane(family, gw, rows, seed), bp.plane(family, gw, rows, seed)
        assert a.dtype == np.bool_ and a.shape == (rows, gw) and np.array_equal(a, b)
        assert not a.flags.writeable and a.any()
        assert not np.array_equal(a, bp.plane(family, gw, rows, seed + 1))
        lr, ud = bp.plane(family + "-lr", gw, rows, seed), bp.plane(family + "-ud", gw, rows, seed)
        assert np.array_equal(lr, a[:, ::-1]) and np.array_equal(ud, a[::-1]) and not lr.flags.writeable and not ud.flags.writeable
        with pytest.raises(ValueError):
            a[0, 0] = True


def test_families_are_what_they_say():
    """The constructions, on the planes themselves (the regimes below are asserted on the model's output)."""
    for gw, rows, seed in ((65, 34, 4), (130, 21, 5)):
        mz = bp.plane("maze", gw, rows, seed)
        nodes = len(range(1, gw - 1, 2)) * len(range(1, rows, 2))
        assert int(mz.sum()) == 2 * nodes - 1 and mz[1::2, 1:gw - 1:2].all()          # a spanning tree: nodes - 1 corridors
        assert not mz[:, 0].any() and not mz[:, gw - 1].any()
        up, down = bp.plane("comb_up", gw, rows, seed), bp.plane("comb_down", gw, rows, seed)
        assert up[rows - 1, 1:gw - 1].all() and down[0, 1:gw - 1].all() and not up[:rows - 1, 2:gw - 1:2].any()
        assert up[rows - 2, 1:gw - 1:2].all() and len(set(up[:, 1:gw - 1:2].sum(axis=0).tolist())) > 3      # teeth, of several lengths
        br = bp.plane("bars", gw, rows, seed)
        assert (br[0::2].sum(axis=1) >= gw - 3).all() and (br[1::2].sum(axis=1) <= 3).all() and br[0::2, 0].all() and br[0::2, gw - 1].all()
        gaps = ~br[0::2]
        assert not (gaps[:, 1:] & gaps[:, :-1]).any()                                  # single cells
        cf = bp.plane("confetti", gw, rows, seed)
        lab = bm.label(cf)
        assert np.bincount(lab.reshape(-1))[1:].tolist() == [3] * int(lab.max()) and not cf[:, 0].any() and not cf[:, gw - 1].any()


def test_plane_frame_is_cells_frame():
    a = bp.plane("perc50", 40, 9, 1)
    ys, xs = np.nonzero(a)
    for shift in (4, 1):
        want = bi.voters([(int(x), int(y), 1, 5, 0) for x, y in zip(xs, ys)], shift)
        assert np.array_equal(bp.plane_frame(a, shift), want)
    assert np.array_equal(bp.plane_frame(a), bi.cells_frame(list(zip(xs.tolist(), ys.tolist()))))


def test_the_case_table():
    """Every grid the issue names, one batch each, smallest first; one frame without side data and one with side data and
    no record in the middle; the wide grid takes bars and percolation, the tall one perc60, the maze and the combs."""
    assert [(g.gw, g.gh, g.margin) for g in bp.GRIDS.values()] == [(63, 12, 0), (64, 12, 0), (65, 34, 0), (128, 20, 0), (129, 20, 0),
                                                                    (120, 68, 3), (2000, 9, 0), (66, 400, 0), (240, 135, 6), (240, 135, 0)]
    assert sorted(bp.GPU_ORDER) == sorted(bp.BATCHES)
    cells = [bp.batch(n).grid.gw * bp.batch(n).grid.gh * (2 if n in bp.MASKED else 1) for n in bp.GPU_ORDER]
    assert cells == sorted(cells)
    for name in bp.BATCHES:
        b = bp.batch(name)
        assert (b.p.grid_w, b.p.grid_h, b.p.vertical_margin, b.p.vectors_needed, b.p.clusters_needed) == (b.grid.gw, b.grid.gh, b.grid.margin, 1, 1)
        F = len(b.names) + 2
        mid = len(b.names) // 2
        n_rec = np.diff(b.off.astype(np.int64))
        assert len(b.sd) == len(b.off) - 1 == (2 * F if name in bp.MASKED else F) and n_rec.max() <= 31000
        assert b.sd[:F].tolist() == [int(f != mid) for f in range(F)] and n_rec[mid] == 0 and n_rec[mid + 1] == 0
        assert sorted(b.frame_of.values()) == [f for f in range(F) if f not in (mid, mid + 1)]
        assert not b.mv.flags.writeable and not b.off.flags.writeable
        assert b.mv.dtype == m.MV_DTYPE and b.mv.dtype.itemsize == 40 and b.mv.flags.c_contiguous     # a pipe is fed these bytes
        assert b.mv.view(np.uint8).reshape(-1, 40)[:, 34:40].any()                                    # junk in the padding
        fams = {n.partition("-")[0] for n in b.names}
        if b.grid.kind == "wide":
            assert fams == set(bp.PERC) | {"bars"} and b.p.block_shift == 1 and (b.grid.gw + 63) // 64 == 32
        elif b.grid.kind == "tall":
            assert fams == {"perc60", "maze", "comb_up", "comb_down"} and b.p.block_shift == 1
        else:
            assert fams == set(ALL_FAMILIES) and len(b.names) == 18 and b.p.block_shift == 4
        for fam in bp.FLIPPED:
            assert (fam in fams) == (fam + "-lr" in b.names) == (fam + "-ud" in b.names)
        if name in bp.MASKED:
            assert b.keeps.shape == (2, b.grid.gh, b.grid.gw) and b.keeps[0].all() and b.soff.tolist() == [0, F, 2 * F]
            assert 0.13 < 1.0 - b.keeps[1].mean() < 0.17
            assert np.array_equal(b.mv[:len(b.mv) // 2], b.mv[len(b.mv) // 2:])
        else:
            assert b.soff is None and b.keeps is None


# ------------------------------------------------------------------ the model against scipy

@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_model_labels_every_plane_as_scipy_does(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    want = bp.expected(name)
    seen = 0
    for _, f, cen in centre_planes(name):
        lab, n = ndimage.label(cen, structure=four)
        mine = bm.label(cen)
        assert int(mine.max()) == n == int(want["blobs"][f])
        # the same partition: the pairs (scipy label, model label) are a bijection
        pairs = set(zip(lab[cen].tolist(), mine[cen].tolist()))
        assert len(pairs) == n and len({a for a, _ in pairs}) == n and len({b for _, b in pairs}) == n
        assert not mine[~cen].any()
        assert int(cen.sum()) == int(want["centres"][f]) and (n == 0 or int(np.bincount(lab.reshape(-1))[1:].max()) == int(want["largest"][f]))
        seen += 1
    assert seen == int(bp.batch(name).sd.sum())


def test_masked_first_stream_reads_the_unmasked_answer():
    """blob_planes.expected() takes the first stream of a masked batch from the grid's own batch; on 120 x 68 the model
    under both planes says the same, and the mask cuts blobs apart."""
    name = "120x68-m3-masked"
    b = bp.batch(name)
    direct = bm.model_batch(b.p, b.mv, b.off, b.sd, b.soff, b.keeps)
    want = bp.expected(name)
    for k in ("centres", "blobs", "largest", "box"):
        assert np.array_equal(direct[k], want[k]), k
    F = len(b.sd) // 2
    for fam in ("maze", "comb_up", "comb_down"):
        f = b.frame_of[fam]
        assert want["blobs"][f] == 1 and want["blobs"][F + f] > 100 and want["centres"][F + f] < want["centres"][f]


# ------------------------------------------------------------------ every family reaches its regime

@pytest.mark.parametrize("name", list(bp.GRIDS))
def test_every_family_reaches_its_regime(name):
    b = bp.batch(name)
    st = lambda n: bp.stats(name, n)                         # noqa: E731
    if "perc35" in b.names:
        c, n, g, _ = st("perc35")
        assert n >= 30
        if (b.grid.gw, b.grid.gh) == (240, 135):
            assert n > 1024                                  # more roots than lanes in the workgroup
    c, n, g, _ = st("perc60")
    if name in bp.BIG:
        assert n >= 50 and g >= 500 and g < c, (name, c, n, g)
    else:
        assert n >= 2 and g < c
    if "perc95" in b.names:
        assert 1 <= st("perc95")[1] <= 3
    for fam in ("maze", "comb_up", "comb_down"):
        if fam in b.names:
            c, n, g, _ = st(fam)
            assert n == 1 and g == c > b.grid.gw, (name, fam, c, n, g)
    if "bars" in b.names:
        c, n, g, _ = st("bars")
        cen = next(cp for pn, _, cp in centre_planes(name) if pn == "bars")
        joined = cen[:-2] & cen[1:-1] & cen[2:]              # a bridge cell with a cell of the bar above and of the bar below
        assert n >= 2 and joined.any(), (name, n)
        lab = bm.label(cen)
        y, x = (int(v[0]) for v in np.nonzero(joined))
        assert lab[y, x] == lab[y + 2, x] != 0
    if "confetti" in b.names:
        c, n, g, box = st("confetti")
        cen = next(cp for pn, _, cp in centre_planes(name) if pn == "confetti")
        lab = bm.label(cen)
        assert g == 3 and n >= 20 and c == 3 * n
        ys, xs = np.nonzero(lab == n)                        # the blob a "last index wins" rule would pick
        last = (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
        ys, xs = np.nonzero(lab == 1)
        assert box == (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())) != last


@pytest.mark.parametrize("name", list(bp.GRIDS))
def test_mirror_images_keep_the_counts_and_move_the_box(name):
    b = bp.batch(name)
    moved = 0
    for fam in bp.FLIPPED:
        if fam not in b.names:
            continue
        base = bp.stats(name, fam)
        for flip in ("-lr", "-ud"):
            got = bp.stats(name, fam + flip)
            assert got[:3] == base[:3], (name, fam + flip)
            moved += got[3] != base[3]
    assert moved >= 1


# ------------------------------------------------------------------ previews and the embedding

def test_both_previews_accept_every_grid():
    for g in bp.GRIDS.values():
        p = bp.params_of(g)
        R = g.gh - 2 * g.margin
        lds, lds_gmc = bp.preview_lds(p)
        assert lds == bi.lds_by_hand(g.gw, R) <= bp.MI355X_LDS, g.name
        assert lds_gmc == lds + 2 * 256 * 4 + 32 <= bp.MI355X_LDS, g.name
        m.plan_preview(p)


@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_pan_embedding_exists_for_every_frame(name):
    """gmc_blobs_inputs.embed returns a batch under the pan of the GPU tier's check 4; the model finds the pan on every
    frame with side data and, on the blob outputs, what the plain model finds on the original batch."""
    b, e = bp.batch(name), bp.embedded(name)
    assert e is not None and e.pan == bp.PAN
    own = np.diff(b.off.astype(np.int64))
    assert all(n > o if s else n == 0 for n, o, s in zip(e.fillers, own, b.sd))
    want, plain = bp.expected_embedded(name), bp.expected(name)
    has = np.flatnonzero(b.sd)
    assert (want["info"][has][:, :2] == bp.PAN).all() and (want["info"][has][:, 2:4] == bp.PAN).all()
    assert not want["info"][np.flatnonzero(b.sd == 0)].any()
    for k in ("centres", "blobs", "largest", "box"):
        assert np.array_equal(want[k], plain[k]), (name, k)
