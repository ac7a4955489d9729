"""The pipe round of a draw of tests/derived_soak.py — what tests/test_gpu_pipe_soak.py feeds to the pipe forms of the
masked scan, the blob scan and the compensated scan (zones_frames_kernel, blobs_frames_kernel and gmc_frames_kernel with
PIPE = true, launched from mtgpu_pipe_submit after mtgpu_pipe_set_keep / set_blobs / set_gmc) — and its expected
values, usable without a GPU (tests/test_pipe_soak_host.py replays the first iterations).

    r = pipe_round(d, seed)                       # d = derived_soak.draw(...): pipe geometry, frames, pipe_mv, keep planes
    e = expected_pipe(d, r, form, keep)           # form in FORMS, keep in (None,) + PLANES; lists in frame order
    d, r = replay(seed, it)                       # iteration `it` of the soak with `seed`, rebuilt on the CPU
    r = seam_round(width, compact, zero_copy)     # the fixed word-seam grids, the same kind of round without a draw

Everything random in a round comes from a fourth RandomState, seeded from (seed, it, PIPE_SALT): the draw, `rng`,
draw_gmc's state and draw_blobs's state are what they were (the digest tests of tests/test_derived_cliff_host.py).

A round takes every frame of its draw: the expected values of the costliest of the default seed's first 60 draws (64
frames, 342 505 records, max_shift 127, five keep planes) take one second of CPU time, the average one 0.1 s, so the
models do not hold the soak under two draws in four seconds and no window of frames is cut.

The record copy pipe_mv lets the MASK decide the vector: a share d["gmc_follow"] of every frame's records follows a pan
— pan A = d["gmc_pans"][f] where the destination cell lies left of the split column c, a second pan B right of it.
Under the plane "left" the masked estimate sees pan A alone, under "right" pan B alone, without a keep both."""
import numpy as np

import mvtrim_amd as m

import blobs_model as bm
import derived_soak as dsoak
import oracle_binding as ob
import pipe_gmc_inputs as pgi
import zones_inputs as zi
from derived_edge_inputs import MI355X_LDS, voters

PIPE_SALT = 0x919E                                       # the fourth state's seed is (seed, it, PIPE_SALT)
DEFAULT_SEED = dsoak.DEFAULT_SEED
FORMS = ("plain", "masked", "blobs", "gmc")
PLANES = ("left", "right", "drawn", "ones")
SEAM_COLUMNS = (63, 64, 65, 127, 128, 129)


def support_of(p):
    """Which setters the pipe accepts on the grid of p: set_keep asks the masked scan's preview (also for the blob scan
    and the compensated scan under a keep), set_blobs the blob scan's, set_gmc the compensated scan's."""
    return {"masked": dsoak._preview(m.zones_preview, p, MI355X_LDS), "blobs": dsoak._preview(m.blobs_preview, p, MI355X_LDS),
            "gmc": dsoak._preview(m.gmc_preview, p, MI355X_LDS)}


def two_pan_copy(p, mv, off, pans_a, pans_b, c, who):
    """A copy of the records in which every record of `who` has its src overwritten with dst - pan, clipped to int16 as
    derived_soak.draw_gmc clips: pan A of its frame where the destination cell's column is below c, pan B otherwise."""
    out = mv.copy()
    fr = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    left = (mv["dst_x"].astype(np.int64) >> p.block_shift) < c
    pan = np.where(left[:, None], np.asarray(pans_a, dtype=np.int64)[fr], np.asarray(pans_b, dtype=np.int64)[fr])
    out["src_x"][who] = np.clip(mv["dst_x"][who].astype(np.int64) - pan[who, 0], -32768, 32767)
    out["src_y"][who] = np.clip(mv["dst_y"][who].astype(np.int64) - pan[who, 1], -32768, 32767)
    return out


def _frames(mv, off, sd):
    """The frames as the pipe can express them: None without side data (the pipe has no "records and no side data"),
    else the frame's records — an empty array for an empty frame with side data."""
    return [None if not sd[f] else np.ascontiguousarray(mv[int(off[f]):int(off[f + 1])]) for f in range(len(sd))]


def _split_planes(gh, gw, c):
    cols = np.arange(gw)[None, :]
    return np.repeat(cols < c, gh, axis=0), np.repeat(cols >= c, gh, axis=0)


def pipe_round(d, seed=DEFAULT_SEED):
    """The pipe round's own inputs of a creatable draw d."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(d["it"]), PIPE_SALT])
    p = d["params"]
    gw, gh = p.grid_w, p.grid_h
    F = len(d["sd"])
    mv, off, sd = d["mv"], d["off"], d["sd"]
    sizes = np.diff(off.astype(np.int64))
    largest, total = int(sizes.max()), int(sizes.sum())
    # geometry
    max_frames = int(rng.choice([1, 3, 7, F, F + 5]))
    kind = str(rng.choice(["growth", "two-mean", "whole"]))
    max_records = {"growth": max(1, largest // 3), "two-mean": max(1, 2 * total // F), "whole": max(1, total)}[kind]
    n_buffers = int(rng.choice([1, 2, 3]))
    zero_copy = bool(rng.rand() < 0.5)
    # the split column: a word seam's neighbourhood where the grid has one
    pool = [x for x in SEAM_COLUMNS if 1 <= x <= gw - 1]
    if pool and rng.rand() < 0.75:
        c = int(rng.choice(pool))
    else:
        c = int(rng.randint(1, max(gw, 2)))
    ms = d["gmc_max_shift"]
    pans_a = np.asarray(d["gmc_pans"], dtype=np.int64)
    pans_b = rng.randint(-(ms + 2), ms + 3, size=(F, 2)).astype(np.int64)
    who = rng.rand(len(mv)) < d["gmc_follow"]
    pipe_mv = two_pan_copy(p, mv, off, pans_a, pans_b, c, who)
    left, right = _split_planes(gh, gw, c)
    planes = {"left": left, "right": right, "ones": np.ones((gh, gw), dtype=bool)}
    if d["keeps"] is not None:
        planes["drawn"] = np.ascontiguousarray(d["keeps"][int(rng.randint(0, len(d["keeps"])))])
    blob_plane = str(rng.choice([k for k in ("left", "right", "drawn") if k in planes]))
    return dict(it=d["it"], seed=seed, params=p, support=support_of(p), F=F, mv=mv, pipe_mv=pipe_mv, off=off, sd=sd,
                frames=_frames(mv, off, sd), frames_gmc=_frames(pipe_mv, off, sd), max_frames=max_frames, max_records=max_records,
                records_kind=kind, growth=max_records < largest, n_buffers=n_buffers, zero_copy=zero_copy, compact=bool(d["compact"]),
                c=c, pans_a=pans_a, pans_b=pans_b, planes=planes, blob_plane=blob_plane, max_shift=ms, share_q8=d["gmc_share_q8"],
                min_blob_cells=d["min_blob_cells"], memo={})


def replay(seed, target):
    d = dsoak.replay(seed, target)
    return d, (pipe_round(d, seed) if d["creatable"] else None)


def layout_of(r):
    return (m.LAYOUT_COMPACT8 if r["compact"] else m.LAYOUT_AOS40) | (m.LAYOUT_ZERO_COPY if r["zero_copy"] else 0) | m.LAYOUT_CENTRES


def where_of(r):
    p = r["params"]
    return (f"pipe round: {r['F']} frames, max_frames {r['max_frames']}, max_records {r['max_records']} "
            f"({r['records_kind']}), n_buffers {r['n_buffers']}, compact {r['compact']}, zero-copy {r['zero_copy']}, split column {r['c']} "
            f"of {p.grid_w} (W {(p.grid_w + 63) // 64}), margin {p.vertical_margin}, max_shift {r['max_shift']}, min_share_q8 {r['share_q8']}, "
            f"min_blob_cells {r['min_blob_cells']}, blob plane {r['blob_plane']}")


def expected_pipe(d, r, form, keep=None, check_sources=False):
    """{"flags", "centres"} lists in frame order of the round r under the plane named `keep` (None: no keep), and
    "largest" (blobs) or "vector" (gmc, packed as MT_PIPE_REPORT_VECTOR packs it).  Only models the repository has:
      plain    oracle_binding.scan_centres
      masked   zones_inputs.model_batch with the one plane as one stream
      blobs    derived_soak.blob_batch, flags by blobs_model.flags_np with the round's min_blob_cells
      gmc      no keep: derived_soak.gmc_counts_np on pipe_mv; under a keep: pipe_gmc_inputs.model
    check_sources: a second, independently written source agrees — masked: the oracle on filtered records
    (vectors_needed >= 1); blobs: the centres are the masked (or plain) form's; gmc without a keep: pipe_gmc_inputs.model;
    gmc under a keep: derived_soak.blob_batch(gmc=..., keeps=[plane]), centres and applied vector.  d may be None."""
    key = (form, keep)
    if key in r["memo"] and not check_sources:
        return r["memo"][key]
    p, off, sd, F, it = r["params"], r["off"], r["sd"], r["F"], r["it"]
    plane = None if keep is None else r["planes"][keep]
    soff = np.array([0, F], dtype=np.uint64)
    cn, ms, q8 = max(1, p.clusters_needed), r["max_shift"], r["share_q8"]
    if form == "plain":
        assert keep is None
        fl, ce = ob.scan_centres(p, r["mv"], off, sd, nthreads=8)
        e = dict(flags=fl.tolist(), centres=ce.tolist())
    elif form == "masked":
        ce = zi.model_batch(p, r["mv"], off, sd, soff, plane[None])[0]
        if check_sources and (p.vectors_needed & 0xFF) >= 1:
            fl, oc, _ = zi.oracle_batch(p, r["mv"], off, sd, soff, plane[None])
            assert oc.tolist() == ce.tolist() and fl.tolist() == (ce >= cn).astype(np.uint8).tolist(), ("masked against the oracle", it, keep)
        e = dict(flags=(ce >= cn).astype(np.uint8).tolist(), centres=ce.tolist())
    elif form == "blobs":
        b = dsoak.blob_batch(p, r["mv"], off, sd, None if plane is None else soff, None if plane is None else plane[None],
                             check_labels=check_sources)
        if check_sources:
            other = expected_pipe(d, r, "plain" if plane is None else "masked", keep)
            assert b["centres"].tolist() == other["centres"], ("blobs against " + ("plain" if plane is None else "masked"), it, keep)
        e = dict(flags=bm.flags_np(p, b["centres"], b["largest"], r["min_blob_cells"]).tolist(), centres=b["centres"].tolist(),
                 largest=b["largest"].tolist())
    else:
        assert form == "gmc"
        if plane is None:
            ce, info = dsoak.gmc_counts_np(p, r["pipe_mv"], off, sd, ms, q8)
            e = dict(flags=(ce >= cn).astype(np.uint8).tolist(), centres=ce.tolist(),
                     vector=[pgi.pack_vector(x, y) for x, y in info[:, :2].tolist()])
            if check_sources:
                fl, mc, mvec = pgi.model(p, r["frames_gmc"], ms, q8)
                assert (fl, mc, mvec) == (e["flags"], e["centres"], e["vector"]), ("gmc, two models", it)
        else:
            fl, ce, vec = pgi.model(p, r["frames_gmc"], ms, q8, plane)
            e = dict(flags=fl, centres=ce, vector=vec)
            if check_sources:
                b = dsoak.blob_batch(p, r["pipe_mv"], off, sd, soff, plane[None], gmc=(ms, q8))
                assert b["centres"].tolist() == ce, ("gmc under a keep, centres", it, keep)
                assert [pgi.pack_vector(x, y) for x, y in b["info"][:, :2].tolist()] == vec, ("gmc under a keep, vector", it, keep)
    r["memo"][key] = e
    return e


def reach(d, r):
    """What the round reaches, from the models alone: booleans by name."""
    p, sup = r["params"], r["support"]
    out = dict(words2=p.grid_w > 64, margin=p.vertical_margin > 0, seam_split=r["c"] % 64 == 0, growth=bool(r["growth"]),
               none_frames=bool((r["sd"] == 0).any()), vector_left_right=False, vector_masked=False, blob_flag_off=False)
    if sup["gmc"] and sup["masked"]:
        free = expected_pipe(d, r, "gmc")["vector"]
        le, ri = expected_pipe(d, r, "gmc", "left")["vector"], expected_pipe(d, r, "gmc", "right")["vector"]
        out["vector_left_right"] = any(a != b and a != 0 and b != 0 for a, b in zip(le, ri))
        under = [le, ri] + ([expected_pipe(d, r, "gmc", "drawn")["vector"]] if "drawn" in r["planes"] else [])
        out["vector_masked"] = any(v != free for v in under)
    if sup["blobs"] and sup["masked"] and r["min_blob_cells"] > 0:
        a, b = expected_pipe(d, r, "blobs")["flags"], expected_pipe(d, r, "blobs", r["blob_plane"])["flags"]
        out["blob_flag_off"] = any(x and not y for x, y in zip(a, b))
    return out


# ------------------------------------------------------------------ the fixed word-seam grids

SEAM_WIDTHS = {1008: 63, 1024: 64, 1040: 65, 2048: 128, 2064: 129}
SEAM_HEIGHT, SEAM_GH, SEAM_MARGIN = 272, 17, 2
SEAM_KW = dict(vertical_mask=0.125, vectors_needed=2, clusters_needed=20, mv_threshold_sq=16.0)
SEAM_MS, SEAM_Q8, SEAM_MIN_BLOB = 16, 100, 15
SEAM_PANS_A = [(5, -3), (-9, 4), (2, 2)]
SEAM_PANS_B = [(-7, 2), (6, 6), (-1, -12)]
SEAM_CLEARED_ROW = 7                                     # an analysed row (2 .. 14)
SEAM_LAYOUTS = [(True, True), (False, False)]            # compact8 + zero-copy; aos40 with a device mirror


def seam_planes(gw, gh=SEAM_GH):
    """{name: bool [gh, gw]}: left and right of the split column (64; 32 where the grid has 63 or 64 columns), only column 63,
    only column 64 (where the grid has them), only the last column — each also with the analysed row SEAM_CLEARED_ROW
    cleared — and all ones."""
    c = 64 if gw > 64 else 32
    left, right = _split_planes(gh, gw, c)
    base = {"left": left, "right": right}
    for name, x in (("col63", 63), ("col64", 64), ("last", gw - 1)):
        if x < gw:
            k = np.zeros((gh, gw), dtype=bool)
            k[:, x] = True
            base[name] = k
    out = {}
    for name, k in base.items():
        out[name] = k
        k2 = k.copy()
        k2[SEAM_CLEARED_ROW] = False
        out[name + "-row"] = k2
    out["ones"] = np.ones((gh, gw), dtype=bool)
    return c, out


def seam_round(width, compact=True, zero_copy=True):
    """A round on the 16-pixel grid of width x 272 (gh 17, margin 2: y_lo 2 > 0, crows 13 < R): three frames of a few
    hundred records — every row of the columns next to column 0, to the split, to the word seams and to the last column,
    three votes a cell, and 40 random cells — in which every other record follows the frame's pan A left of the split
    column and pan B right of it, the others move at random."""
    gw = SEAM_WIDTHS[width]
    p = m.ScanParams.from_config(width, SEAM_HEIGHT, **SEAM_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (gw, SEAM_GH, SEAM_MARGIN, 4)
    c, planes = seam_planes(gw)
    rng = np.random.RandomState(width)
    cols = sorted({x for x in (0, 1, 2, c - 2, c - 1, c, c + 1, 62, 63, 64, 65, 126, 127, 128, gw - 3, gw - 2, gw - 1) if 0 <= x < gw})
    frames = []
    for f in range(3):
        cells = [(x, y, 3, 0, 0) for y in range(SEAM_GH) for x in cols]
        cells += [(int(rng.randint(0, gw)), int(rng.randint(0, SEAM_GH)), int(rng.randint(1, 4)), 0, 0) for _ in range(40)]
        fr = voters(cells, 4)
        fr["src_x"] = fr["dst_x"] - rng.randint(-20, 21, size=len(fr))
        fr["src_y"] = fr["dst_y"] - rng.randint(-20, 21, size=len(fr))
        frames.append(fr[rng.permutation(len(fr))])
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    mv = np.ascontiguousarray(np.concatenate(frames), dtype=m.MV_DTYPE)
    sd = np.ones(3, dtype=np.uint8)
    who = rng.rand(len(mv)) < 0.5
    pipe_mv = two_pan_copy(p, mv, off, SEAM_PANS_A, SEAM_PANS_B, c, who)
    total = int(off[-1])
    return dict(it=f"seam grid {width}", seed=None, params=p, support=support_of(p), F=3, mv=mv, pipe_mv=pipe_mv, off=off, sd=sd,
                frames=_frames(mv, off, sd), frames_gmc=_frames(pipe_mv, off, sd), max_frames=2, max_records=total, records_kind="whole",
                growth=False, n_buffers=2, zero_copy=zero_copy, compact=compact, c=c, pans_a=np.array(SEAM_PANS_A), pans_b=np.array(SEAM_PANS_B),
                planes=planes, blob_plane="left", max_shift=SEAM_MS, share_q8=SEAM_Q8, min_blob_cells=SEAM_MIN_BLOB, memo={})
