"""The random stream of tests/test_gpu_derived_soak.py — the soak of the sweep, the activity map, the masked scan, the
compensated scan, the blob scan, the compensated blob scan, the direction scan, the plane scan and the flow map — and
its expected values, usable without a GPU
(tests/test_derived_cliff_host.py replays the first iterations).  The two labelling kernels meet any grid width and
height here, with the LDS layout that follows from it; random connectivity is the business of tests/test_gpu_blob_planes.py.

    d = draw(rng, it, seed)           # grid, parameters, batch, streams, masks, settings, record layout, base alignment
    e = expected(d, kernel)           # kernel in KERNELS, where d["support"][kernel]
    d = replay(seed, it)              # iteration `it` of the soak with `seed`, rebuilt on the CPU

What the compensated scan alone needs (max_shift, min_share_q8, a pan per frame and its own copy of the records, in which
a share of every frame's records follows the pan) comes from a RandomState of its own, seeded from (seed, it): the
stream `rng` and everything drawn from it are what they were before that kernel joined.  What the two blob scans alone
need (min_blob_cells, whether the call is masked) comes from a third RandomState, seeded from (seed, it) and BLOBS_SALT:
`rng` and draw_gmc's state are what they were before the blob scans joined.  The blob scan runs on d["mv"], the
compensated one on d["gmc_mv"] with draw_gmc's settings; masked, both use d["zsoff"] and d["keeps"].  What the direction
scan, the plane scan and the flow map alone need (an allow byte, bytes per stream, planes, the forms of the two calls)
comes from a fourth RandomState, seeded from (seed, it) and DIR_SALT: the three states before it are what they were.
All three run on d["mv"]; the per-stream forms use d["zsoff"] (frames may lie behind the last stream), the flow map
d["soff"].

The grid comes from w, h in [64, 3900] x [64, 2200] and block_shift 1 .. 5 as in tests/soak_replay.py, but the shifts are
not equally likely: a derived kernel holds a whole frame's counters in LDS and supports about 37 000 cells, which a
grid of 2- or 4-pixel cells rarely stays under.  With the weights of SHIFT_P each kernel is supported in at least three
quarters of the draws (asserted on the CPU); the rest checks that an unsupported grid is refused and touches nothing."""
import numpy as np

import mvtrim_amd as m
from mvtrim_amd import _abi, synth

import blobs_model as bm
import dir_model as dm
import gmc_blobs_inputs as gbi
import gmc_model as gm
import lanes_model as lm
import oracle_binding as ob
import pipe_gmc_inputs as pgi
import zones_inputs as zi
from activity_model import assert_oracle_identities, model_maps
from derived_edge_inputs import MI355X_LDS, UNALIGNED_SHIFTS
from scan_checks import junk_padding

KERNELS = ("sweep", "activity", "zones", "gmc", "blobs", "gmc_blobs", "dir", "lanes", "flow")
DEFAULT_SEED = 24680
SHIFT_P = [0.04, 0.08, 0.18, 0.35, 0.35]                 # block_shift 1 .. 5
THR_POOL = [0.0, 4.0, 9.5, 16.0, 25.0, 37.0, 4294967296.0, float("inf")]
VEC_POOL = [0, 1, 2, 3, 4, 6, 12, 255]
GMC_SHIFT_POOL = [0, 1, 6, 16, 127]
GMC_SHARE_Q8_POOL = [0, 77, 128, 256]
GMC_FOLLOW_POOL = [0.0, 0.4, 0.6, 0.95]                  # the share of a frame's records that follow its pan
GMC_SHIFT_P = [0.1, 0.15, 0.25, 0.3, 0.2]
GMC_SHARE_Q8_P = [0.25, 0.3, 0.3, 0.15]
GMC_FOLLOW_P = [0.1, 0.25, 0.3, 0.35]
BLOBS_SALT = 0xB10B                                      # the third state's seed is (seed, it, BLOBS_SALT); draw_gmc's is (seed, it)
MIN_BLOB_POOL = [0, 1, 2, 3, 5, 12, 40, 3000]            # 0 and 1 change no flag; 40 and 3000 lie above most blobs' sizes
DIR_SALT = 0xD12                                         # the fourth state's seed is (seed, it, DIR_SALT)
# nothing, everything, single sectors, halves and mixed bytes.  The blobs of zones_inputs.clustered_frame all move east
# (bit 0): most of the pool forbids that, which is what turns flags off.
ALLOW_POOL = [0x00, 0xFF, 0x01, 0x02, 0x10, 0x80, 0x55, 0xAA, 0x0F, 0xF0, 0xA4, 0x3C, 0xDA, 0xFE]
PLANE_KINDS = ("bytes", "density", "all")                # random bytes; 0x00 / 0xFF at a drawn density; all 0xFF
PLANE_KIND_P = [0.5, 0.35, 0.15]
PLANE_DENSITY_POOL = [0.0, 0.3, 0.9]                     # the share of 0xFF cells of a "density" plane


def _preview(fn, *a):
    try:
        fn(*a)
        return True
    except m.MtgpuError as e:
        assert e.code == _abi.MT_ERR_UNSUPPORTED, e
        return False


def support_of(p, n_thr, n_vec, lds=MI355X_LDS):
    return {"sweep": _preview(m.sweep_preview, p, n_thr, n_vec, lds), "activity": _preview(m.activity_preview, p, lds),
            "zones": _preview(m.zones_preview, p, lds)}


def draw_gmc(seed, it, p, mv, off):
    """The compensated scan's own inputs of iteration `it`: max_shift, min_share_q8, a pan (a, b) per frame within
    +-(max_shift + 2) — some fall outside the bins — and gmc_mv, a copy of the records in which a share of every frame's
    records has its src overwritten with dst - pan, clipped to int16."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(it)])
    ms = int(rng.choice(GMC_SHIFT_POOL, p=GMC_SHIFT_P))
    q8 = int(rng.choice(GMC_SHARE_Q8_POOL, p=GMC_SHARE_Q8_P))
    F = len(off) - 1
    pans = rng.randint(-(ms + 2), ms + 3, size=(F, 2)).astype(np.int64)
    follow = float(rng.choice(GMC_FOLLOW_POOL, p=GMC_FOLLOW_P))
    out = mv.copy()
    fr = np.repeat(np.arange(F), np.diff(off.astype(np.int64)))
    who = rng.rand(len(mv)) < follow
    out["src_x"][who] = np.clip(mv["dst_x"][who].astype(np.int64) - pans[fr[who], 0], -32768, 32767)
    out["src_y"][who] = np.clip(mv["dst_y"][who].astype(np.int64) - pans[fr[who], 1], -32768, 32767)
    return dict(gmc_max_shift=ms, gmc_share_q8=q8, gmc_pans=pans, gmc_follow=follow, gmc_mv=out,
                support_gmc=_preview(m.gmc_preview, p, MI355X_LDS))


def draw_blobs(seed, it, p):
    """The blob scans' own inputs of iteration `it`: min_blob_cells, and whether the two calls carry the draw's streams and
    keep masks (they run unmasked where the draw has no masks: see blob_masks)."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(it), BLOBS_SALT])
    return dict(min_blob_cells=int(rng.choice(MIN_BLOB_POOL)), blob_masked=bool(rng.rand() < 0.5),
                support_blobs=_preview(m.blobs_preview, p, MI355X_LDS), support_gmc_blobs=_preview(m.gmc_blobs_preview, p, MI355X_LDS))


def draw_dir(seed, it, p, n_streams):
    """The inputs of the direction scan, the plane scan and the flow map of iteration `it`: a scalar allow byte; whether
    the direction call is per-stream and its bytes (one per stream of d["zsoff"]); the planes uint8 [S, gh, gw] of those
    streams — each random bytes, 0x00 / 0xFF at a drawn density, or all 0xFF — where the plane scan supports the grid
    (None elsewhere: a refused call reads no plane); whether the plane call uses the one-plane form (planes[0] for every
    frame)."""
    rng = np.random.RandomState([int(seed) & 0xFFFFFFFF, int(it), DIR_SALT])
    out = dict(allow=int(rng.choice(ALLOW_POOL)), dir_per_stream=bool(rng.rand() < 0.5),
               allows=rng.choice(ALLOW_POOL, size=n_streams).astype(np.uint8), lanes_one_plane=bool(rng.rand() < 0.35),
               support_dir=_preview(m.dir_preview, p, MI355X_LDS), support_lanes=_preview(m.lanes_preview, p, MI355X_LDS),
               planes=None, plane_kinds=None)
    if out["support_lanes"]:
        kinds = [str(k) for k in rng.choice(PLANE_KINDS, size=n_streams, p=PLANE_KIND_P)]
        planes = np.full((n_streams, p.grid_h, p.grid_w), 0xFF, dtype=np.uint8)
        for i, kind in enumerate(kinds):
            if kind == "bytes":
                planes[i] = rng.randint(0, 256, size=(p.grid_h, p.grid_w))
            elif kind == "density":
                planes[i] = np.where(rng.rand(p.grid_h, p.grid_w) < float(rng.choice(PLANE_DENSITY_POOL)), 0xFF, 0x00)
        out.update(planes=planes, plane_kinds=kinds, lanes_staged=m.lanes_preview(p, MI355X_LDS)["staged"])
    return out


def dir_args(d):
    """The keyword arguments of dir_model.model_batch for the draw's direction call."""
    return dict(soff=d["zsoff"], allows=d["allows"]) if d["dir_per_stream"] else dict(allow=d["allow"])


def lanes_args(d):
    """(planes, stream_off) of the draw's plane call."""
    return (d["planes"][0], None) if d["lanes_one_plane"] else (d["planes"], d["zsoff"])


def blob_masks(d):
    """(stream_off, keeps) of the blob scans' calls on draw d, or (None, None): unmasked by the draw, or masked by the
    draw on a grid the masked scan does not support, for which no keeps were drawn."""
    return (d["zsoff"], d["keeps"]) if d["blob_masked"] and d["keeps"] is not None else (None, None)


def draw(rng, it, seed=DEFAULT_SEED):
    """One iteration's inputs.  "creatable": False where mtgpu_create refuses the grid (nothing else is drawn then)."""
    sh = int(rng.choice([1, 2, 3, 4, 5], p=SHIFT_P))
    w, h = int(rng.randint(64, 3900)), int(rng.randint(64, 2200))
    kw = dict(mv_threshold_sq=float(rng.choice([16.0, 4.0, 0.0, 9.5, 4294967296.0], p=[0.3, 0.3, 0.15, 0.15, 0.1])),
              block_size=1 << sh, block_shift=sh,
              vectors_needed=int(rng.choice([1, 1, 2, 2, 3, 4, 6, 12, 255, 0])),
              clusters_needed=int(rng.choice([1, 2, 2, 3, 10])),
              vertical_mask=float(rng.choice([0.0, 0.05, 0.2, 0.5], p=[0.4, 0.3, 0.2, 0.1])))
    p = ob.params_from_config(w, h, **kw)
    d = dict(it=it, w=w, h=h, kw=kw, params=p, creatable=True)
    try:
        m.plan_preview(p)
    except m.MtgpuError as e:
        assert e.code == _abi.MT_ERR_CAPACITY
        d.update(creatable=False, support={k: False for k in KERNELS}, mv=np.zeros(0, dtype=m.MV_DTYPE))
        return d
    # the sweep's settings, unsorted, with duplicates
    thr = [float(x) for x in rng.choice(THR_POOL, size=int(rng.randint(1, 9)))]
    vec = [int(x) for x in rng.choice(VEC_POOL, size=int(rng.randint(1, 9)))]
    support = support_of(p, len(thr), len(vec))
    # the batch: ragged random frames with blobs added, so that centres exist; runs on every other iteration
    F = int(rng.choice([3, 9, 17, 40, 64]))
    fewer = 1 if any(support.values()) else 8                # nothing reads the records of a grid no kernel supports
    mv, off, _ = synth.random_frames(rng, F, int(rng.choice([200, 3000, 8000])) // fewer, w, h, hot=float(rng.choice([0.05, 0.5, 0.95])))
    n_blobs = int(rng.choice([0, 4, 12, 30]))
    frames = [np.concatenate([mv[int(off[f]):int(off[f + 1])], zi.clustered_frame(rng, p, n_blobs + f % 3)]) for f in range(F)]
    frames = [f[rng.permutation(len(f))] for f in frames]
    if rng.rand() < 0.3:
        frames[int(rng.randint(0, F))] = np.zeros(0, dtype=m.MV_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
    mv = np.ascontiguousarray(np.concatenate(frames), dtype=m.MV_DTYPE)
    if it % 2 == 0 and len(mv):                              # tests/soak_replay.py, draw_tail: every record 1 .. 6 times
        r = rng.randint(1, 7, size=len(mv))
        csum = np.concatenate([[0], np.cumsum(r)])
        off = csum[off.astype(np.int64)].astype(np.uint64)
        mv = np.repeat(mv, r)
    junk_padding(mv, rng)
    sd = (rng.rand(F) < 0.85).astype(np.uint8)
    # streams: 1 .. 5 at random cut points, empty ones allowed; the masked scan sometimes leaves frames behind the last
    S = int(rng.randint(1, 6))
    soff = np.array([0] + sorted(int(x) for x in rng.randint(0, F + 1, size=S - 1)) + [F], dtype=np.uint64)
    behind = int(rng.choice([0, 0, 1, 2]))
    zsoff = np.minimum(soff, F - behind).astype(np.uint64)
    dens = [float(x) for x in rng.choice([0.0, 0.3, 0.9, 1.0], size=S)]
    keeps = np.stack([rng.rand(p.grid_h, p.grid_w) < q for q in dens]) if support["zones"] else None
    window = None
    if it % 3 == 0:
        window = (int(rng.choice(UNALIGNED_SHIFTS)), 8 * int(rng.randint(0, 16)))     # 40-byte shift, compact residue
    d.update(support=support, mv=mv, off=off, sd=sd, thr=thr, vec=vec, soff=soff, zsoff=zsoff, keep_density=dens, keeps=keeps,
             min_centres=int(rng.choice([0, 1, 2])), run_frames=int(rng.choice([0, 1, 3, 17])), compact=bool(it % 2), window=window)
    g = draw_gmc(seed, it, p, mv, off)                       # not from `rng`: see the module docstring
    support["gmc"] = g.pop("support_gmc")
    d.update(g)
    b = draw_blobs(seed, it, p)                              # nor from draw_gmc's state
    support["blobs"], support["gmc_blobs"] = b.pop("support_blobs"), b.pop("support_gmc_blobs")
    d.update(b)
    g = draw_dir(seed, it, p, S)                             # nor from draw_blobs' state
    support["dir"], support["lanes"] = g.pop("support_dir"), g.pop("support_lanes")
    support["flow"] = support["lanes"]                       # the flow map answers with the plane scan's plan
    d.update(g)
    return d


def replay(seed, target):
    rng = np.random.RandomState(seed)
    for it in range(1, target + 1):
        d = draw(rng, it, seed)
    return d


def _setting_params(d, thr, vec):
    kw = dict(d["kw"], mv_threshold_sq=thr, vectors_needed=vec)
    return ob.params_from_config(d["w"], d["h"], **kw)


def sweep_counts_np(p, mv, off, sd, thrs, vecs):
    """{(thr, vec): uint32 [F]}: the centre counts of every setting by the numpy rule, restated here for a block of
    settings (zones_inputs.zone_counts_np states it for one): per frame one histogram per threshold — kept records with a
    destination cell on an analysed row — saturated at 255, `>= vec` per level, and a centre is an active cell of an
    analysed row and an inner column with an active 4-neighbour.  A frame without side data counts 0."""
    gw, gh, mg, F = p.grid_w, p.grid_h, p.vertical_margin, len(sd)
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    out = {(t, v): np.zeros(F, dtype=np.uint32) for t in thrs for v in vecs}
    for f in range(F):
        if not sd[f]:
            continue
        r = mv[int(off[f]):int(off[f + 1])]
        d2 = ((r["dst_x"].astype(np.int64) - r["src_x"]) ** 2 + (r["dst_y"].astype(np.int64) - r["src_y"]) ** 2).astype(np.float64)
        gx, gy = r["dst_x"].astype(np.int64) >> p.block_shift, r["dst_y"].astype(np.int64) >> p.block_shift
        inside = (gx >= 0) & (gx < gw) & (gy >= 0) & (gy < gh)
        inside &= rows[np.clip(gy, 0, gh - 1), 0]
        cell = gy * gw + gx
        for t in thrs:
            ok = inside & ~(d2 < t)
            votes = np.minimum(np.bincount(cell[ok], minlength=gw * gh).reshape(gh, gw), 255)
            for v in vecs:
                act = votes >= (v & 0xFF)
                z = np.pad(act, 1)
                nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
                out[t, v][f] = int((act & nb & rows)[:, 1:gw - 1].sum())
    return out


def zones_vn0_count(p, keep):
    """The masked centre count of ANY frame with side data under vectors_needed 0, cell by cell in plain Python (the
    records play no part): a cell of the grid is active iff its row is not analysed or its keep bit is set; a centre is
    an active cell of an analysed row, x in [1, gw - 2], with an active 4-neighbour inside the grid."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    lo, hi = min(mg, gh), max(gh - mg, min(mg, gh))
    keep = np.asarray(keep, dtype=bool).tolist()

    def active(x, y):
        return 0 <= x < gw and 0 <= y < gh and (not lo <= y < hi or keep[y][x])
    n = 0
    for y in range(lo, hi):
        for x in range(1, gw - 1):
            n += active(x, y) and (active(x - 1, y) or active(x + 1, y) or active(x, y - 1) or active(x, y + 1))
    return int(n)


def gmc_counts_np(p, mv, off, sd, max_shift, min_share_q8):
    """(centres uint32 [F], info rows int64 [F, 7] in the order gx, gy, mode_x, mode_y, n_in, n_x, n_y): include/mtgpu_gmc.h
    restated for a batch with one bincount per histogram — the bins in the order of the walk 0, -1, +1, ..., the first
    maximum of that row is the mode — and one bincount for the residual votes.  A frame without side data reads 0."""
    gw, gh, mg, F = p.grid_w, p.grid_h, p.vertical_margin, len(sd)
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    order = np.array(gm.walk(max_shift), dtype=np.int64) + max_shift
    thr = gm.threshold_int(p.mv_threshold_sq)
    centres, info = np.zeros(F, dtype=np.uint32), np.zeros((F, 7), dtype=np.int64)
    for f in range(F):
        if not sd[f]:
            continue
        r = mv[int(off[f]):int(off[f + 1])]
        d = [r["dst_x"].astype(np.int64) - r["src_x"], r["dst_y"].astype(np.int64) - r["src_y"]]
        cx, cy = r["dst_x"].astype(np.int64) >> p.block_shift, r["dst_y"].astype(np.int64) >> p.block_shift
        inside = (cx >= 0) & (cx < gw) & (cy >= mg) & (cy < gh - mg)
        n_in = int(inside.sum())
        g = [0, 0]
        for ax in (0, 1):
            v = d[ax][inside]
            h = np.bincount(v[np.abs(v) <= max_shift] + max_shift, minlength=2 * max_shift + 1)[order]
            o = int(np.argmax(h))                            # the first maximum in walk order
            mode, n = int(order[o]) - max_shift, int(h[o])
            g[ax] = mode if n * 256 >= min_share_q8 * n_in else 0
            info[f, 2 + ax], info[f, 5 + ax] = mode, n
        info[f, 0], info[f, 1], info[f, 4] = g[0], g[1], n_in
        votes = np.zeros((gh, gw), dtype=np.int64)
        if thr is not None and n_in:
            rx, ry = d[0] - g[0], d[1] - g[1]
            ok = inside & (rx * rx + ry * ry >= thr)
            votes = np.bincount((cy * gw + cx)[ok], minlength=gw * gh).reshape(gh, gw)
        act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
        z = np.pad(act, 1)
        nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
        centres[f] = int((act & nb & rows)[:, 1:gw - 1].sum())
    return centres, info


def _same_partition(cen, lab):
    """blobs_model.label's partition of the plane is scipy.ndimage.label's (4-neighbourhood); True where scipy is absent."""
    try:
        from scipy import ndimage
    except ImportError:
        return True
    ref, n = ndimage.label(cen, structure=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))
    pairs = set(zip(ref[cen].tolist(), lab[cen].tolist()))
    return int(lab.max()) == n == len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs}) and not lab[~cen].any()


def blob_batch(p, mv, off, sd, soff=None, keeps=None, gmc=None, check_labels=False):
    """blobs_model.model_batch (gmc None) or gmc_blobs_inputs.model_batch (gmc = (max_shift, min_share_q8)), frame for
    frame and line for line, with blobs_model.blob_stats memoised per distinct centre plane: under vectors_needed 0 the
    64 frames of a draw share one plane per stream — one blob of up to 37 000 cells, seconds of flood fill each.  Every
    frame is still checked.  check_labels: every distinct plane's labelling is also held against scipy's."""
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else np.zeros(F, dtype=np.int64)
    out = {k: np.zeros(F, dtype=np.uint32) for k in ("centres", "blobs", "largest")}
    out["box"] = np.full((F, 4), 0xFFFF, dtype=np.uint16)
    if gmc is not None:
        out["info"] = np.zeros((F, 7), dtype=np.int64)
    memo = {}
    for f in range(F):
        if not has[f] or (keeps is not None and not 0 <= st[f] < len(keeps)):
            continue
        fr, keep = mv[int(off[f]):int(off[f + 1])], None if keeps is None else keeps[st[f]]
        if gmc is None:
            cen = bm.centre_plane(p, fr, keep)
        else:
            gx, gy, n_in, mx, nx, my, ny = pgi.estimate(p, fr, gmc[0], gmc[1], keep)
            cen = gbi.centre_plane(p, fr, gx, gy, keep)
            out["info"][f] = (gx, gy, mx, my, n_in, nx, ny)
        key = np.packbits(cen).tobytes()
        if key not in memo:
            memo[key] = bm.blob_stats(cen)
            assert not check_labels or _same_partition(cen, bm.label(cen)), ("labelling", f)
        out["centres"][f], out["blobs"][f], out["largest"][f], out["box"][f] = memo[key]
    return out


def _expected_blobs(d, kernel, check_sources):
    """The expected outputs of the blob scan (on d["mv"]) or the compensated blob scan (on d["gmc_mv"]) under
    blob_masks(d), and what the draw reaches: "multi" (frames with more than one blob), "flag_off" (frames whose centre
    count alone would set the flag and whose largest blob is below min_blob_cells), "flag_kept" (frames flagged under a
    min_blob_cells above 1), "masked", "behind" (frames behind the last stream of a masked call).  check_sources: the
    memoised batch equals the model's own model_batch; masked, the blob scan's centres are the masked scan's expected
    ones under the same streams and keeps, unmasked the oracle's; unmasked, the compensated form's centres and info are
    the compensated scan's expected ones; every distinct plane labels as scipy labels it."""
    p, off, sd = d["params"], d["off"], d["sd"]
    soff, keeps = blob_masks(d)
    if kernel == "blobs":
        mv, gmc = d["mv"], None
    else:
        mv, gmc = d["gmc_mv"], (d["gmc_max_shift"], d["gmc_share_q8"])
    e = blob_batch(p, mv, off, sd, soff, keeps, gmc, check_labels=check_sources)
    if check_sources:
        model = bm.model_batch(p, mv, off, sd, soff, keeps) if gmc is None else gbi.model_batch(p, mv, off, sd, gmc[0], gmc[1], soff, keeps)
        for k in e:
            assert e[k].tolist() == model[k].tolist(), (kernel, k, d["it"])
        if gmc is None and keeps is not None:
            assert e["centres"].tolist() == zi.model_batch(p, mv, off, sd, soff, keeps)[0].tolist(), ("blobs against zones", d["it"])
        elif gmc is None:
            assert e["centres"].tolist() == ob.scan_centres(p, mv, off, sd, nthreads=8)[1].tolist(), ("blobs against the oracle", d["it"])
        elif keeps is None:
            ce, rows = expected(d, "gmc")["centres"], expected(d, "gmc")["info"]
            assert e["centres"].tolist() == ce.tolist() and e["info"].tolist() == rows.tolist(), ("gmc_blobs against gmc", d["it"])
    mb, cn = d["min_blob_cells"], max(1, p.clusters_needed)
    e["flags"] = bm.flags_np(p, e["centres"], e["largest"], mb)
    by_count = e["centres"] >= cn
    e.update(total=int(e["centres"].sum(dtype=np.uint64)), multi=int((e["blobs"] > 1).sum()),
             flag_off=int((by_count & (e["flags"] == 0)).sum()), flag_kept=int((e["flags"] != 0).sum()) if mb > 1 else 0,
             masked=keeps is not None, behind=int(len(sd) - int(soff[-1])) if keeps is not None else 0)
    return e


def plain_scan(d):
    """(flags, centres) of the oracle on the draw's records as they are: what allow 0xFF and a plane of 0xFF must give.
    Computed once per draw."""
    if "_plain" not in d:
        d["_plain"] = ob.scan_centres(d["params"], d["mv"], d["off"], d["sd"], nthreads=8)
    return d["_plain"]


def _expected_dir(d, kernel, check_sources):
    """The expected outputs of the direction scan or the plane scan on d["mv"], "plain" (plain_scan) and what the draw
    reaches: "flag_off" (frames inside a stream whose plain flag is set and which the byte or plane turns off),
    "per_stream" (the form with one byte or plane per stream of d["zsoff"]), "behind" (frames behind its last stream).
    check_sources: the oracle on filtered records (consequence C), or under vectors_needed 0, where that oracle has no
    level 0, consequence F against the plain scan; the roses' sums against dir_model.counting_moving (B)."""
    p, mv, off, sd = d["params"], d["mv"], d["off"], d["sd"]
    F = len(sd)
    if kernel == "dir":
        kw, per_stream = dir_args(d), d["dir_per_stream"]
        fl, ce, rose = dm.model_batch(p, mv, off, sd, **kw)
        owned = dm.frame_allows(F, d["allow"], kw.get("soff"), kw.get("allows")) >= 0
    else:
        (planes, soff), per_stream = lanes_args(d), not d["lanes_one_plane"]
        fl, ce, rose = lm.model_batch(p, mv, off, sd, planes, soff)
        owned = lm.frame_planes(F, planes, soff) >= 0
    pf, pc = plain_scan(d)
    if check_sources:
        if (p.vectors_needed & 0xFF) == 0:
            assert ce[owned].tolist() == pc[owned].tolist() and not ce[~owned].any(), (kernel, "consequence F", d["it"])
        else:
            ofl, oce = dm.oracle_batch(p, mv, off, sd, **kw) if kernel == "dir" else lm.oracle_batch(p, mv, off, sd, planes, soff)
            assert oce.tolist() == ce.tolist() and ofl.tolist() == fl.tolist(), (kernel, "consequence C", d["it"])
        assert rose.sum(axis=1).tolist() == np.where(owned, dm.counting_moving(p, mv, off, sd), 0).tolist(), (kernel, "B", d["it"])
    return dict(flags=fl, centres=ce, rose=rose, plain=(pf, pc), total=int(ce.sum(dtype=np.uint64)) + int(pc.sum(dtype=np.uint64)),
                flag_off=int((owned & (pf != 0) & (fl == 0)).sum()), per_stream=per_stream, behind=int((~owned).sum()) if per_stream else 0)


def expected(d, kernel, check_sources=False):
    """The expected outputs of `kernel` on draw d and "total", the sum of the centre counts they hold.  check_sources:
    assert that the second, independent source agrees — the sweep: the oracle and sweep_counts_np on every setting; the
    activity map: the numpy model and the oracle's identities; the masked scan (always checked): the numpy AND rule
    against the oracle on filtered records, or under vectors_needed 0 against zones_vn0_count, and centres_all against
    the oracle on the records as they are; the compensated scan (on d["gmc_mv"]): gmc_counts_np against tests/gmc_model.py
    with its candidate-by-candidate mode_of, and consequence C of include/mtgpu_gmc.h against the oracle on every frame
    whose src + (gx, gy) stays in int16.  The compensated scan adds "compensated" (frames with gx or gy != 0),
    "compensated_with_centres" and "found_not_applied" (a mode != 0 on an axis whose g is 0).  The two blob scans:
    _expected_blobs.  The direction scan and the plane scan: _expected_dir; their "total" adds the plain scan's counts,
    which the GPU run also holds allow 0xFF and a plane of 0xFF to.  The flow map (on d["soff"]): lanes_model.flow_map,
    "total" its sum; check_sources: per stream its sums are the sums of the roses of the stream's frames (G)."""
    p, mv, off, sd = d["params"], d["mv"], d["off"], d["sd"]
    if kernel == "gmc":
        mv, ms, q8 = d["gmc_mv"], d["gmc_max_shift"], d["gmc_share_q8"]
        ce, rows = gmc_counts_np(p, mv, off, sd, ms, q8)
        if check_sources:
            _, mc, mi = gm.gmc_batch(p, mv, off, sd, ms, q8)
            assert mc.tolist() == ce.tolist(), ("gmc centres", d["it"])
            assert np.stack([mi[k].astype(np.int64) for k in mi.dtype.names], axis=1).tolist() == rows.tolist(), ("gmc info", d["it"])
            fits = np.array([gm.shift_src(mv, off[f:f + 2], rows[f:f + 1, 0], rows[f:f + 1, 1]) is not None for f in range(len(sd))])
            moved = gm.shift_src(mv, off, np.where(fits, rows[:, 0], 0), np.where(fits, rows[:, 1], 0))
            oc = ob.scan_centres(p, moved, off, sd, nthreads=8)[1]
            assert oc[fits].tolist() == ce[fits].tolist(), ("gmc consequence C", d["it"])
        comp = (rows[:, 0] != 0) | (rows[:, 1] != 0)
        lost = ((rows[:, 2] != 0) & (rows[:, 0] == 0)) | ((rows[:, 3] != 0) & (rows[:, 1] == 0))
        return dict(flags=(ce >= max(1, p.clusters_needed)).astype(np.uint8), centres=ce, info=rows, total=int(ce.sum(dtype=np.uint64)),
                    compensated=int(comp.sum()), compensated_with_centres=int((comp & (ce > 0)).sum()), found_not_applied=int(lost.sum()))
    if kernel in ("blobs", "gmc_blobs"):
        return _expected_blobs(d, kernel, check_sources)
    if kernel in ("dir", "lanes"):
        return _expected_dir(d, kernel, check_sources)
    if kernel == "flow":
        flow = lm.flow_map(p, mv, off, sd, d["soff"])
        if check_sources:
            rose = dm.model_batch(p, mv, off, sd)[2]
            for st in range(len(d["soff"]) - 1):
                a, b = int(d["soff"][st]), int(d["soff"][st + 1])
                assert flow[st].sum(axis=(1, 2)).tolist() == rose[a:b].sum(axis=0, dtype=np.uint64).tolist(), ("flow G", d["it"], st)
        return dict(flow=flow, total=int(flow.sum(dtype=np.uint64)))
    if kernel == "sweep":
        T, V, F = len(d["thr"]), len(d["vec"]), len(sd)
        want, memo = np.zeros((T, V, F), dtype=np.uint32), {}
        for t, thr in enumerate(d["thr"]):
            for v, vec in enumerate(d["vec"]):
                if (thr, vec) not in memo:
                    memo[thr, vec] = ob.scan_centres(_setting_params(d, thr, vec), mv, off, sd, nthreads=8)[1]
                want[t, v] = memo[thr, vec]
        if check_sources:                                    # the numpy rule on every distinct setting of the block
            model = sweep_counts_np(p, mv, off, sd, sorted({t for t, _ in memo}), sorted({v for _, v in memo}))
            for key, oracle in memo.items():
                assert oracle.tolist() == model[key].tolist(), ("sweep", d["it"], key)
        return dict(centres=want, total=int(want.sum(dtype=np.uint64)))
    if kernel == "activity":
        a, c, fr, counts = model_maps(p, mv, off, sd, d["soff"], d["min_centres"])
        if check_sources:
            oc = assert_oracle_identities(p, mv, off, sd, d["soff"], d["min_centres"], c, fr, ("activity", d["it"]))
            assert np.array_equal(oc[sd != 0], counts[sd != 0])
        return dict(maps=(a, c, fr), total=int(counts.sum()))
    assert kernel == "zones"
    soff, keeps = d["zsoff"], d["keeps"]
    mc, mca = zi.model_batch(p, mv, off, sd, soff, keeps)
    oca = ob.scan_centres(p, mv, off, sd, nthreads=8)[1].copy()
    oca[zi.stream_of_frames(soff, len(sd)) >= len(keeps)] = 0
    assert np.array_equal(oca, mca), ("zones centres_all", d["it"])
    if (p.vectors_needed & 0xFF) == 0:                       # the oracle on filtered records has no vectors_needed 0:
        per_stream = [zones_vn0_count(p, k) for k in keeps]  # zones_vn0_count stands in for it     
        st = zi.stream_of_frames(soff, len(sd))
        loop = [per_stream[st[f]] if sd[f] and 0 <= st[f] < len(keeps) else 0 for f in range(len(sd))]
        assert mc.tolist() == loop, ("zones centres, vectors_needed 0", d["it"])
    else:
        fl, oc, _ = zi.oracle_batch(p, mv, off, sd, soff, keeps)
        assert np.array_equal(oc, mc), ("zones centres", d["it"])
        assert np.array_equal(fl, (mc >= max(1, p.clusters_needed)).astype(np.uint8))
    return dict(flags=(mc >= max(1, p.clusters_needed)).astype(np.uint8), centres=mc, centres_all=mca,
                total=int(mca.sum(dtype=np.uint64)))
