"""Inputs of tests/test_gpu_derived_cliff.py: the grids on which the sweep, the activity map, the masked scan, the
compensated scan, the direction scan and the plane scan fill their LDS to the last row or column, found with the previews (host arithmetic, no GPU), and a
small batch for each with the values derived BY HAND from its construction.  tests/test_derived_cliff_host.py proves
without a GPU that every shape sits on the limit, that the batches carry centres and that two independent expected-value sources agree on them.

Every shape has vertical_mask 0 (R = grid_h) and block_shift 1, which keeps every pixel coordinate inside int16 — but for
the sweep's two-column grids: 20 000 rows of two-pixel cells reach past 32 767, so those two use block_shift 0, where a
pixel coordinate is the cell index itself.  Nothing below is a literal size; bisection over the previews at import time
(under functools.lru_cache) finds, at 163 840 bytes of LDS per workgroup:

    kernel        gw=2   gw=3   gw=65  gw=193  | gh=1    gh=3    (largest gh / largest gw; one more is MT_ERR_UNSUPPORTED)
    zones         5118   4548   530    186     | 12722   7572
    activity      6824   5849   559    194     | 13105   7800
    sweep 1 x 1   20442  13627  626    209     | 13217   8028
    sweep 8 x 8   20422  13614  625    208     | 10896   7104
    gmc           10108  8086   584    199     | 13069   7841
    dir           10234  8187   591    201     | 13234   7939
    lanes staged  9096   7119   478    162     | 12244   6931    (one more is supported and reads the plane from memory)
    lanes         10234  8187   591    201     | 13234   7939    (the unstaged form needs what the direction scan needs)

    activity at gw = 120 (every plan outcome is reachable there; the rows are the largest gh of the outcome and, as the
    row after it, the smallest gh that no longer has it — both are shapes):
    32-bit two per CU 54 | 16-bit two per CU 81 | 32-bit alone 110 | 16-bit alone 164 | no accumulators 318 | 319: none

(A record of what the bisection found when this was written; no code reads it.)  gw = 3 is not asked for by
anything but the rule for centres: a column in [1, gw - 2] exists from gw = 3 on, so the two-column grids — five keep
words per lane in the masked scan — can hold active cells and no centre; the three-column ones can hold both.

The batch of a shape (12 frames) is made of
    E   pairs of neighbouring cells in the four corners, on the first and last row, in the first and last column and
        across the row where the masked scan's keep staging starts its second trip (word 1024)
    H   horizontal pairs across the grid's 64-cell word seams — the first, a middle and the last one on wide grids
        (three and four columns: the right corners, which touch the left corners' pairs of E)
    VL  vertical pairs in the column left of those seams,  VR  in the column right of them
    B.  30 blobs of zones_inputs.clustered_frame, anywhere in the grid
    N   a blob frame without side data,  Z  a frame with side data and no record
with junk in the padding bytes of the 40-byte records.

Hand values.  Every pair of a planted frame (E, H, VL, VR) is ISOLATED: no cell of it equals or touches (4-neighbourhood)
a cell of another pair of that frame — plant() refuses a pair that would.  Both cells of pair i get k = 2 + i % 3 votes of
|d|^2 = 25 (i even) or 9 (i odd).  So under a threshold T and a level V >= 1
    a pair is active iff k >= V and |d|^2 >= T, each of its cells then has exactly one active neighbour, the other one,
    and it adds one centre per cell whose column lies in [1, gw - 2]  (vertical_mask 0: every row is analysed);
    with one cell ignored by a keep mask the other cell has no active neighbour left: the pair adds 0;
    at level 0 every cell of the grid is active, whatever the records: gh * (gw - 2) centres from gw = 3 on
    (gh = 1: the horizontal neighbours suffice), in the frame without records too.
hand_count() is that rule and nothing else.

The direction scan and the plane scan get the same pairs with a sector each (the directed planting); their hand values
are stated in front of that section, at the end of this module."""
import dataclasses
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import _abi

import dir_model as dm
import lanes_model as lm
import oracle_binding as ob
import zones_inputs as zi
from derived_edge_inputs import MI355X_LDS, frozen, sweep_chunk_rows, voters
from scan_checks import junk_padding

KERNELS = ("zones", "activity", "sweep1", "sweep8", "gmc", "dir", "lanes")
TALL_GW = (2, 3, 65, 193)
WIDE_GH = (1, 3)
ACT_GW = 120
# (acc_bits, two workgroups per CU) in the order activity_plan falls through them as the grid grows
ACT_OUTCOMES = ((32, True), (16, True), (32, False), (16, False), (0, False))
KEEP_TRIP = 1024                      # lanes of zones_frames_kernel: keep word 1024 is the first of the second trip


# ------------------------------------------------------------------ the grids

def shift_of(gw, gh):
    return 1 if (max(gw, gh) << 1) <= 32767 else 0


def grid_params(gw, gh, **kw):
    sh = shift_of(gw, gh)
    p = m.ScanParams.from_config(gw << sh, gh << sh, block_size=1 << sh, block_shift=sh, vertical_mask=0.0, **kw)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (gw, gh, 0, sh)
    return p


def kernel_preview(kernel, p, lds=MI355X_LDS):
    """The kernel's own preview -> its dict, or None where it answers MT_ERR_UNSUPPORTED (any other error raises)."""
    try:
        if kernel == "zones":
            return m.zones_preview(p, lds)
        if kernel == "activity":
            return m.activity_preview(p, lds)
        if kernel == "gmc":
            return m.gmc_preview(p, lds)
        if kernel == "dir":
            return m.dir_preview(p, lds)
        if kernel == "lanes":
            return m.lanes_preview(p, lds)
        n = 1 if kernel == "sweep1" else 8
        return m.sweep_preview(p, n, n, lds)
    except m.MtgpuError as e:
        if e.code != _abi.MT_ERR_UNSUPPORTED:
            raise
        return None


def creatable(p):
    try:
        m.plan_preview(p)
        return True
    except m.MtgpuError as e:
        assert e.code == _abi.MT_ERR_CAPACITY
        return False


def largest(ok, hi=32767):
    """The largest n in [1, hi] with ok(n), for an ok() that holds up to some n and not beyond."""
    assert ok(1)
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


@functools.lru_cache(maxsize=None)
def tallest(kernel, gw):
    return largest(lambda gh: kernel_preview(kernel, grid_params(gw, gh)) is not None)


@functools.lru_cache(maxsize=None)
def widest(kernel, gh):
    def ok(gw):
        p = grid_params(gw, gh)
        return creatable(p) and kernel_preview(kernel, p) is not None
    return largest(ok, 16383)


def lanes_staged(p):
    pv = kernel_preview("lanes", p)
    return pv is not None and pv["staged"] == 1


@functools.lru_cache(maxsize=None)
def tallest_staged(gw):
    return largest(lambda gh: lanes_staged(grid_params(gw, gh)))


@functools.lru_cache(maxsize=None)
def widest_staged(gh):
    return largest(lambda gw: creatable(grid_params(gw, gh)) and lanes_staged(grid_params(gw, gh)), 16383)


def act_outcome(gh, gw=ACT_GW):
    """Index into ACT_OUTCOMES of the plan of a gw x gh grid; len(ACT_OUTCOMES) where the map is unsupported."""
    pv = kernel_preview("activity", grid_params(gw, gh))
    return len(ACT_OUTCOMES) if pv is None else ACT_OUTCOMES.index((pv["acc_bits"], 2 * pv["lds_bytes"] <= MI355X_LDS))


@functools.lru_cache(maxsize=None)
def act_last(outcome):
    return largest(lambda gh: act_outcome(gh) <= outcome)


@functools.lru_cache(maxsize=None)
def shapes(kernel):
    """{name: (gw, gh, kind)}; kind "tall": one more is gh + 1, "wide": gw + 1, "plan": a plan outcome of the activity
    map that is not the last one — one more row is supported and has the next outcome — or a grid of the plane scan
    around the end of its staged form: "tall-staged" / "wide-staged", the last grid whose plane rows fit next to the
    tile, and "tall-unstaged" / "wide-unstaged", one row or column further, the first one that reads the plane from
    memory.  (The plane scan's "tall" and "wide" shapes are the last unstaged grids: the direction scan's.)"""
    out = {}
    for gw in TALL_GW:
        if kernel == "lanes":
            out[f"tall-staged-{gw}x{tallest_staged(gw)}"] = (gw, tallest_staged(gw), "plan")
            out[f"tall-unstaged-{gw}x{tallest_staged(gw) + 1}"] = (gw, tallest_staged(gw) + 1, "plan")
        out[f"tall-{gw}x{tallest(kernel, gw)}"] = (gw, tallest(kernel, gw), "tall")
    for gh in WIDE_GH:
        if kernel == "lanes":
            out[f"wide-staged-{widest_staged(gh)}x{gh}"] = (widest_staged(gh), gh, "plan")
            out[f"wide-unstaged-{widest_staged(gh) + 1}x{gh}"] = (widest_staged(gh) + 1, gh, "plan")
        out[f"wide-{widest(kernel, gh)}x{gh}"] = (widest(kernel, gh), gh, "wide")
    if kernel == "activity":
        for i, (bits, two) in enumerate(ACT_OUTCOMES):
            last = i == len(ACT_OUTCOMES) - 1
            out[f"plan-{bits}bit-{'two' if two else 'one'}-{ACT_GW}x{act_last(i)}"] = (ACT_GW, act_last(i), "tall" if last else "plan")
            if not last:
                out[f"plan-past-{bits}bit-{'two' if two else 'one'}-{ACT_GW}x{act_last(i) + 1}"] = (ACT_GW, act_last(i) + 1, "plan")
    return out


def one_more(gw, gh, kind):
    return (gw + 1, gh) if kind == "wide" else (gw, gh + 1)


def grows(name):
    """"wide" or "tall": the way a shape of that name grows, whatever its kind."""
    return name.split("-")[0]


# The LDS formulas, restated from the layout comments of csrc/zones_kernels.h, csrc/activity_kernels.h,
# csrc/sweep_kernels.h, csrc/gmc_kernels.h, csrc/dir_kernels.h and csrc/lanes_kernels.h (tile: (R + 2) x gw 32-bit counters
# padded to 16 bytes; W 64-bit words per mask row; the compensated scan: the tile, one plane of R + 2 mask rows, two
# histograms of 256 bins, eight result words; the direction scan: the tile, one plane of R + 2 mask rows, four words of
# totals and the eight of the rose; the plane scan: the same and, staged, R x gw plane bytes padded to 16).  A grid past
# the limit has no preview to ask, so "what one more row or column would add" comes from these; the host test holds
# them to the previews' lds_bytes on every shape.
def _tile(gw, R):
    return 4 * (((R + 2) * gw + 3) & ~3)


def lds_need(kernel, gw, gh):
    """The LEAST the kernel needs on a gw x gh grid (vertical_mask 0): zones and the compensated scan have one form; the
    activity map's smallest is the one without accumulators; the sweep's is one tile and the three-row mask buffer per
    level; the plane scan's is the unstaged form, which is the direction scan's."""
    W = (gw + 63) // 64
    if kernel == "zones":
        return _tile(gw, gh) + (3 * gh + 4) * W * 8 + 16
    if kernel == "activity":
        return _tile(gw, gh) + (2 * gh + 2) * W * 8 + 16
    if kernel == "gmc":
        return _tile(gw, gh) + (gh + 2) * W * 8 + 2 * 256 * 4 + 32
    if kernel in ("dir", "lanes"):
        return _tile(gw, gh) + (gh + 2) * W * 8 + 16 + 32
    return _tile(gw, gh) + (1 if kernel == "sweep1" else 8) * 3 * W * 8 + 256


def act_lds(gw, gh, bits):
    return lds_need("activity", gw, gh) + 2 * gh * ((gw + 3) & ~3) * bits // 8


def lanes_lds(gw, gh, staged):
    """csrc/lanes_kernels.h: the direction scan's LDS and, staged, the gh x gw bytes of the plane's rows padded to 16."""
    return lds_need("lanes", gw, gh) + (((gh * gw + 15) & ~15) if staged else 0)


# ------------------------------------------------------------------ planted pairs

def seams_of(gw):
    """The seams s (columns 64 s - 1 | 64 s) the planted pairs sit on: all of them, or the first, a middle and the last."""
    last = (gw - 1) // 64
    return sorted({s for s in (1, (last + 1) // 2, last) if 1 <= s <= last}) if last > 3 else list(range(1, last + 1))


def plant(candidates, gw, gh):
    """[((xa, ya), (xb, yb))] -> the pairs that lie in the grid and are isolated from the ones taken before them."""
    taken, cells = [], set()
    for a, b in candidates:
        if not all(0 <= x < gw and 0 <= y < gh for x, y in (a, b)) or a == b:
            continue
        near = {(x + dx, y + dy) for x, y in (a, b) for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))}
        if near & cells:
            continue
        taken.append((a, b))
        cells |= {a, b}
    return taken


def planted_frames(gw, gh):
    """{"E" | "H" | "VL" | "VR": [pairs]} (see the module docstring).  Rows of the seam pairs: spread over the grid."""
    W = (gw + 63) // 64
    trip = KEEP_TRIP // W                                     # keep word 1024 is word (1024 % W) of this row
    xm, ym = gw // 2, gh // 2
    E = [((0, 0), (1, 0)), ((gw - 2, 0), (gw - 1, 0)), ((0, gh - 1), (1, gh - 1)), ((gw - 2, gh - 1), (gw - 1, gh - 1)),
         ((xm, 0), (xm + 1, 0)), ((xm + 3, gh - 1), (xm + 4, gh - 1)),                  # first and last row
         ((0, ym), (0, ym + 1)), ((gw - 1, ym + 3), (gw - 1, ym + 4)),                  # first and last column
         ((0, gh - 2), (0, gh - 1)), ((gw - 1, 0), (gw - 1, 1)),                        # corners again, vertically (narrow grids)
         ((min(1, gw - 1), trip - 1), (min(1, gw - 1), trip)), ((gw - 2, trip + 2), (gw - 1, trip + 2)),
         ((xm, 2 * trip - 1), (xm, 2 * trip)), ((xm, 4 * trip - 1), (xm, 4 * trip))]
    H, VL, VR = [], [], []
    for i, s in enumerate(seams_of(gw)):
        y = (gh - 1) * (i + 1) // (len(seams_of(gw)) + 1)
        H += [((64 * s - 1, y), (64 * s, y)), ((64 * s - 1, (y + trip) % gh), (64 * s, (y + trip) % gh))]
        VL += [((64 * s - 1, y), (64 * s - 1, y + 1)), ((64 * s - 1, trip - 1), (64 * s - 1, trip))]
        VR += [((64 * s, y), (64 * s, y + 1)), ((64 * s, trip - 1), (64 * s, trip))]
    if 3 <= gw <= 4:                  # the right corners touch the left corners' pairs: they go to the seamless grid's empty H
        H += [((gw - 1, 0), (gw - 1, 1)), ((gw - 1, gh - 2), (gw - 1, gh - 1))]
    return {n: plant(c, gw, gh) for n, c in (("E", E), ("H", H), ("VL", VL), ("VR", VR))}


def pair_votes(i):
    return 2 + i % 3


def pair_d(i):
    return 5 if i % 2 == 0 else 3


def pairs_records(pairs, shift):
    return voters([(x, y, pair_votes(i), pair_d(i), 0) for i, pr in enumerate(pairs) for x, y in pr], shift)


def hand_count(pairs, gw, gh, thr, level, cleared=()):
    """Centres of a planted frame by the rule of the module docstring.  cleared: cells a keep mask ignores (the rule for
    level 0 is stated without a mask: no caller combines the two)."""
    if level == 0:
        assert not cleared
        return gh * (gw - 2) if gw >= 3 else 0
    n = 0
    for i, pr in enumerate(pairs):
        if pair_votes(i) >= level and not pair_d(i) ** 2 < thr and not set(pr) & set(cleared):
            n += sum(1 for x, _ in pr if 1 <= x <= gw - 2)
    return n


# ------------------------------------------------------------------ the batch of a shape

ORDER = ("E", "B1", "H", "N", "B2", "B3", "E", "H", "VL", "VR", "B4", "Z")
N_BLOBS = 30
ZONE_SOFF = (0, 4, 7, 12)            # stream 0: all ones; 1: 30 % cleared at random; 2: one cell of every seam pair cleared
ACT_SOFF = (0, 6, 12)                # two streams split mid-batch
ACT_RUN = 4                          # runs [0, 4) [4, 8) ...: the stream boundary at 6 lies inside the second one


@functools.lru_cache(maxsize=None)
def batch(gw, gh):
    """(mv, off, sd, planted): the 12 frames of ORDER (E and H appear twice, for the masked scan's streams)."""
    return _batch(gw, gh, planted_frames(gw, gh), pairs_records)


def _batch(gw, gh, planted, records):
    """The batch of a shape with `planted` pairs turned into records by `records`.  The random stream sees the pairs'
    record counts alone: two plantings with the same counts share their blob frames, permutations and padding."""
    sh = shift_of(gw, gh)
    p = grid_params(gw, gh)
    rng = np.random.RandomState(gw * 40009 + gh)
    frames, sd = [], []
    for name in ORDER:
        if name in planted:
            f = records(planted[name], sh)
        elif name == "Z":
            f = np.zeros(0, dtype=m.MV_DTYPE)
        else:
            f = zi.clustered_frame(rng, p, N_BLOBS)
        frames.append(f[rng.permutation(len(f))])
        sd.append(0 if name == "N" else 1)
    b = m.FrameBatch.from_frames(frames)
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    return frozen(mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), np.array(sd, dtype=np.uint8)) + (planted,)


def frames_named(name):
    return [i for i, n in enumerate(ORDER) if n == name]


# the context of the masked scan and of the activity map: every planted pair (k >= 2, |d|^2 >= 9) and every blob cell
# with two votes or more (|d|^2 = 25) is active; the blobs' still records (|d|^2 = 2) are not kept
CTX_KW = dict(vectors_needed=2, mv_threshold_sq=4.0, clusters_needed=2)


# ------------------------------------------------------------------ zones

@functools.lru_cache(maxsize=None)
def zones_case(name):
    """(params, mv, off, sd, soff, keeps bool [3, gh, gw], hand {frame: (centres, centres_all)}).  CTX_KW: every planted
    pair is active.  Stream 2 ignores the LEFT cell of the horizontal seam pairs and the UPPER
    cell of the vertical ones: its three seam frames count 0, and centres_all still counts them."""
    gw, gh, _ = shapes("zones")[name]
    p = grid_params(gw, gh, **CTX_KW)
    mv, off, sd, planted = batch(gw, gh)
    keeps = np.ones((3, gh, gw), dtype=bool)
    keeps[1] = np.random.RandomState(gw + gh).rand(gh, gw) >= 0.3
    cleared = [pr[0] for n in ("H", "VL", "VR") for pr in planted[n]]
    for x, y in cleared:
        keeps[2, y, x] = False
    st = zi.stream_of_frames(ZONE_SOFF, len(ORDER))
    hand = {}
    for f, n in enumerate(ORDER):
        if n in planted and st[f] != 1:
            full = hand_count(planted[n], gw, gh, 4.0, 2)
            hand[f] = (hand_count(planted[n], gw, gh, 4.0, 2, cleared=cleared) if st[f] == 2 else full, full)
    return (p, mv, off, sd) + frozen(np.array(ZONE_SOFF, dtype=np.uint64), keeps) + (hand,)


def zones_expected(p, mv, off, sd, soff, keeps):
    """((flags, centres, centres_all) of the oracle on filtered records, (centres, centres_all) of the numpy AND rule)."""
    return zi.oracle_batch(p, mv, off, sd, soff, keeps), zi.model_batch(p, mv, off, sd, soff, keeps)


# ------------------------------------------------------------------ activity

@functools.lru_cache(maxsize=None)
def activity_case(name):
    gw, gh, _ = shapes("activity")[name]
    mv, off, sd, planted = batch(gw, gh)
    return (grid_params(gw, gh, **CTX_KW),) + (mv, off, sd) + frozen(np.array(ACT_SOFF, dtype=np.uint64)) + (planted,)


@functools.lru_cache(maxsize=None)
def activity_planted_case(name):
    """(mv, off, sd, soff, hand active [1, gh, gw], hand centre, hand frames): the four planted frames alone, one stream.
    Every cell of a pair is active in its frame (CTX_KW) and a centre iff its column lies
    in [1, gw - 2]; a cell reads the number of planted frames that hold it."""
    gw, gh, _ = shapes("activity")[name]
    planted = planted_frames(gw, gh)
    sh = shift_of(gw, gh)
    b = m.FrameBatch.from_frames([pairs_records(planted[n], sh) for n in ("E", "H", "VL", "VR")])
    active, centre = np.zeros((1, gh, gw), dtype=np.uint32), np.zeros((1, gh, gw), dtype=np.uint32)
    for n in ("E", "H", "VL", "VR"):
        for pr in planted[n]:
            for x, y in pr:
                active[0, y, x] += 1
                centre[0, y, x] += 1 <= x <= gw - 2
    return frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
                  np.ones(4, dtype=np.uint8), np.array([0, 4], dtype=np.uint64), active, centre, np.array([4], dtype=np.uint32))


# ------------------------------------------------------------------ sweep

# the caller's order, neither ascending nor descending, 25.0 and level 3 twice, levels 0 and 255
THR8 = [25.0, 9.5, 26.0, 9.0, 0.0, 25.0, 4.0, 4294967296.0]
VEC8 = [2, 0, 255, 3, 1, 4, 3, 5]
CALLS1 = [([16.0], [2]), ([9.0], [0]), ([25.0], [255]), ([9.5], [3])]          # 1 x 1: one call per setting


def sweep_calls(kernel):
    return CALLS1 if kernel == "sweep1" else [(THR8, VEC8)]


@functools.lru_cache(maxsize=None)
def sweep_setting(gw, gh, thr, vec):
    """(oracle counts [F], numpy counts [F]) of one setting on the shape's batch."""
    mv, off, sd, _ = batch(gw, gh)
    p = grid_params(gw, gh, mv_threshold_sq=thr, vectors_needed=vec)
    ones = np.ones((gh, gw), dtype=bool)
    model = np.array([zi.zone_counts_np(p, mv[int(off[f]):int(off[f + 1])], ones)[1] if sd[f] else 0 for f in range(len(sd))],
                     dtype=np.uint32)
    return frozen(ob.scan_centres(p, mv, off, sd, nthreads=4)[1].copy(), model)


def sweep_expected(kernel, name, thr, vec, which=0):
    gw, gh, _ = shapes(kernel)[name]
    return np.stack([np.stack([sweep_setting(gw, gh, float(t), int(v))[which] for v in vec]) for t in thr])


def sweep_hand(kernel, name, thr, vec):
    """{frame: uint32 [T, V]} of the planted frames."""
    gw, gh, _ = shapes(kernel)[name]
    planted = batch(gw, gh)[3]
    return {f: np.array([[hand_count(planted[n], gw, gh, t, v & 0xFF) for v in vec] for t in thr], dtype=np.uint32)
            for f, n in enumerate(ORDER) if n in planted}


def sweep_path(kernel, name):
    """(passes, chunk_rows, R) of the shape's plan."""
    gw, gh, _ = shapes(kernel)[name]
    n = 1 if kernel == "sweep1" else 8
    ch, R, _, pv = sweep_chunk_rows(grid_params(gw, gh), n, n)
    return pv["passes"], ch, R


# ------------------------------------------------------------------ the compensated scan

GMC_SETTINGS = ((0, 128), (16, 128))          # (max_shift, min_share_q8): the plain scan (consequence A), and the default
GMC_PAN = (7, -3)
GMC_PAN_KW = dict(vectors_needed=3, mv_threshold_sq=16.0, clusters_needed=2)   # pairs of 3 votes and more with |d|^2 = 25
GMC_PAN_MAX_SHIFT = 16                        # the pairs' own displacements, 7 + 5 and 7 + 3, are inside the bins


@functools.lru_cache(maxsize=None)
def gmc_expected(gw, gh, ms, q8):
    """(flags, centres, info rows int64 [F, 7]) of tests/gmc_model.py on the shape's batch under CTX_KW."""
    import gmc_inputs as gi
    import gmc_model as gm
    mv, off, sd, _ = batch(gw, gh)
    fl, ce, info = gm.gmc_batch(grid_params(gw, gh, **CTX_KW), mv, off, sd, ms, q8)
    return frozen(fl, ce, gi.info_rows(info))


def gmc_oracle_c(gw, gh, info_rows):
    """Consequence C: (frames checked bool [F], the oracle's plain counts of the batch with (gx, gy) added to every src).
    A frame whose shifted src leaves int16 is not checked (its records keep their src)."""
    import gmc_model as gm
    mv, off, sd, _ = batch(gw, gh)
    F = len(sd)
    fits = np.array([gm.shift_src(mv, off[f:f + 2], info_rows[f:f + 1, 0], info_rows[f:f + 1, 1]) is not None for f in range(F)])
    moved = gm.shift_src(mv, off, np.where(fits, info_rows[:, 0], 0), np.where(fits, info_rows[:, 1], 0))
    return fits, ob.scan_centres(grid_params(gw, gh, **CTX_KW), moved, off, sd, nthreads=4)[1].copy()


def gmc_filler_rows(gh):
    return sorted({0, gh // 2, gh - 1})


@functools.lru_cache(maxsize=None)
def gmc_pan_case(name):
    """(params, mv, off, sd, hand centres uint32 [2], hand info rows int64 [2, 7]): two frames, the pairs of planted
    frame E and of planted frame H, every pair moving by (pair_d(i) + 7, -3), on top of fillers moving by the pan (7, -3)
    in every cell of the first, a middle and the last row (vertical_mask 0: every row is analysed).

    The rule the hand values follow.  The mode is the pan on both axes — the fillers outnumber the pair records
    (asserted) and every record moves by -3 on y — and it is supported: n_x = the fillers > n / 2.  A pair's residual is
    (pair_d(i), 0), so a pair counts what it counts in the plain scan of its own frame: hand_count, unchanged.  A
    filler's residual is (0, 0) and the threshold is 16 > 0: a filler casts NO vote, wherever it lies, so the fillers
    share rows and cells with the pairs (on the corners they must: both sit on the first and the last row) without
    touching the count.  One filler per cell, but for the grids of two and three columns, where three rows hold fewer
    cells than the pairs hold records: there every cell gets the smallest number of fillers that outnumbers them."""
    gw, gh, _ = shapes("gmc")[name]
    sh = shift_of(gw, gh)
    p = grid_params(gw, gh, **GMC_PAN_KW)
    assert p.mv_threshold_sq > 0.0
    planted = planted_frames(gw, gh)
    rng = np.random.RandomState(gw * 7 + gh)
    frames, centres, info = [], [], []
    for n in ("E", "H"):
        pairs = planted[n]
        pr = voters([(x, y, pair_votes(i), pair_d(i) + GMC_PAN[0], GMC_PAN[1]) for i, q in enumerate(pairs) for x, y in q], sh)
        cells = [(x, y) for y in gmc_filler_rows(gh) for x in range(gw)]
        per_cell = 1 + len(pr) // len(cells)
        fill = voters([(x, y, per_cell) + GMC_PAN for x, y in cells], sh)
        assert len(fill) > len(pr) and (per_cell == 1 or gw <= 3), (name, n, len(fill), len(pr))
        f = np.concatenate([pr, fill])
        frames.append(f[rng.permutation(len(f))])
        centres.append(hand_count(pairs, gw, gh, 16.0, 3))
        info.append(GMC_PAN + GMC_PAN + (len(f), len(fill), len(f)))
    b = m.FrameBatch.from_frames(frames)
    mv = np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy()
    junk_padding(mv, rng)
    return (p,) + frozen(mv, np.ascontiguousarray(b.frame_off, dtype=np.uint64), np.ones(2, dtype=np.uint8),
                         np.array(centres, dtype=np.uint32), np.array(info, dtype=np.int64))


# ------------------------------------------------------------------ the direction scan and the plane scan
#
# The directed planting: the pairs of planted_frames() on the ANALYSED rows (all of them, but for a phase variant with a
# margin), both cells of pair i with pair_votes(i) records of displacement dir_inputs.DISP[i % 8] — sector i % 8,
# |d|^2 = 25 or 32 — in the batch of _batch(): blob frames (every record moves east), N, Z, junk padding.  Under CTX_KW
# every pair passes the threshold and the level.  Hand values:
#   the rose of a planted frame   bin s = the sum over the pairs with i % 8 == s of 2 pair_votes(i), whatever is allowed
#   the direction scan, byte A    pair i adds one centre per cell with its column in [1, gw - 2] iff bit i % 8 of A is
#                                 set (a pair whose sector is forbidden casts no vote: both cells are inactive and, being
#                                 isolated, take no other pair's centre with them); A = 0xFF: hand_count
#   the plane scan                P_all: 0xFF everywhere: hand_count.  P_own: both cells of pair i hold 1 << (i % 8), every
#                                 other cell 0x00: every pair votes: hand_count.  P_half: the first cell of pair i holds
#                                 0xFF ^ (1 << (i % 8)), the second 1 << (i % 8), every other cell 0xFF: the first cell
#                                 casts no vote, the second has no active neighbour left: 0.
#   the flow map of a frame       cell (x, y) of pair i holds pair_votes(i) in sector i % 8, every other word 0
# P_own and P_half take their bytes from the pairs of E and then from the pairs of H that share no cell with them (on
# three and four columns H holds the right corners): the first and the last cell of the first and the last analysed row
# hold a byte of their own wherever the grid has room for the corner pairs.  The hand values of P_own and P_half are
# stated for E, and for H where all of its pairs got their bytes; the other frames' expected values are the model's.
# hand_dir_count(), hand_rose(), hand_flow() and lanes_hand() are those rules and nothing else.

DIR_CHAIN = (0x00, 0x55, 0xAA, 0xFF)           # nothing; E, S, W, N; SE, SW, NW, NE; everything
DIR_STREAM_ALLOWS = (0x0F, 0xA5, 0xD2)         # one byte per stream of ZONE_SOFF
LANES_ROTATIONS = (("all", "own", "half"), ("half", "all", "own"), ("own", "half", "all"))   # plane of stream 0, 1, 2


def directed_records(pairs, shift):
    from dir_inputs import DISP          # not at the top: dir_inputs imports the soak, whose blob inputs import this module
    return voters([(x, y, pair_votes(i)) + tuple(DISP[i % 8]) for i, pr in enumerate(pairs) for x, y in pr], shift)


def with_margin(p, margin):
    return dataclasses.replace(p, vertical_margin=margin) if margin else p


@functools.lru_cache(maxsize=None)
def dir_batch(gw, gh, margin=0):
    """(mv, off, sd, planted) with the directed planting on rows margin .. gh - margin - 1."""
    planted = {n: [tuple((x, y + margin) for x, y in pr) for pr in prs] for n, prs in planted_frames(gw, gh - 2 * margin).items()}
    return _batch(gw, gh, planted, directed_records)


def hand_rose(pairs):
    rose = np.zeros(8, dtype=np.uint32)
    for i in range(len(pairs)):
        rose[i % 8] += 2 * pair_votes(i)
    return rose


def hand_dir_count(pairs, gw, allow):
    return sum(sum(1 for x, _ in pr if 1 <= x <= gw - 2) for i, pr in enumerate(pairs) if (allow >> (i % 8)) & 1)


def hand_flow(pairs, gw, gh):
    flow = np.zeros((8, gh, gw), dtype=np.uint32)
    for i, pr in enumerate(pairs):
        for x, y in pr:
            flow[i % 8, y, x] = pair_votes(i)
    return flow


@functools.lru_cache(maxsize=None)
def dir_case(name):
    """dict: params, mv, off, sd, planted, soff (ZONE_SOFF), allows (DIR_STREAM_ALLOWS)."""
    gw, gh, _ = shapes("dir")[name]
    mv, off, sd, planted = dir_batch(gw, gh)
    return dict(params=grid_params(gw, gh, **CTX_KW), mv=mv, off=off, sd=sd, planted=planted,
                soff=frozen(np.array(ZONE_SOFF, dtype=np.uint64))[0], allows=frozen(np.array(DIR_STREAM_ALLOWS, dtype=np.uint8))[0])


@functools.lru_cache(maxsize=None)
def dir_expected(name, allow=None):
    """The model's (flags, centres, rose) of the shape's batch under one byte, or (None) under the case's streams."""
    c = dir_case(name)
    kw = dict(soff=c["soff"], allows=c["allows"]) if allow is None else dict(allow=allow)
    return frozen(*dm.model_batch(c["params"], c["mv"], c["off"], c["sd"], **kw))


def dir_hand(c, allow=None):
    """{frame: (centres, rose)} of the planted frames under one byte, or under the case's streams."""
    st = zi.stream_of_frames(c["soff"], len(ORDER))
    gw = c["params"].grid_w
    return {f: (hand_dir_count(c["planted"][n], gw, int(c["allows"][st[f]]) if allow is None else allow), hand_rose(c["planted"][n]))
            for f, n in enumerate(ORDER) if n in c["planted"]}


def pair_planes(gw, gh, planted):
    """({"all", "own", "half": uint8 [gh, gw]}, the planted frames whose every pair got its bytes)."""
    own, half = np.zeros((gh, gw), dtype=np.uint8), np.full((gh, gw), 0xFF, dtype=np.uint8)
    taken, whole = set(), []
    for n in ("E", "H"):
        placed = 0
        for i, (a, b) in enumerate(planted[n]):
            if {a, b} & taken:
                continue
            taken |= {a, b}
            placed += 1
            bit = 1 << (i % 8)
            own[a[1], a[0]] = own[b[1], b[0]] = bit
            half[a[1], a[0]], half[b[1], b[0]] = 0xFF ^ bit, bit
        if placed == len(planted[n]):
            whole.append(n)
    return dict(zip(("all", "own", "half"), frozen(np.full((gh, gw), 0xFF, dtype=np.uint8), own, half))), tuple(whole)


@functools.lru_cache(maxsize=None)
def lanes_case(name, margin=0):
    """dict: params, mv, off, sd, planted, soff (ZONE_SOFF), planes {"all", "own", "half"}, whole, R (analysed rows)."""
    gw, gh, _ = shapes("lanes")[name]
    mv, off, sd, planted = dir_batch(gw, gh, margin)
    planes, whole = pair_planes(gw, gh, planted)
    return dict(params=with_margin(grid_params(gw, gh, **CTX_KW), margin), mv=mv, off=off, sd=sd, planted=planted,
                soff=frozen(np.array(ZONE_SOFF, dtype=np.uint64))[0], planes=planes, whole=whole, R=gh - 2 * margin)


def lanes_stack(c, rotation):
    return np.stack([c["planes"][k] for k in rotation])


@functools.lru_cache(maxsize=None)
def lanes_expected(name, rotation, margin=0):
    c = lanes_case(name, margin)
    return frozen(*lm.model_batch(c["params"], c["mv"], c["off"], c["sd"], lanes_stack(c, rotation), c["soff"]))


def lanes_hand(c, rotation):
    """{frame: (centres or None where the rule above states none, rose)} of the planted frames."""
    st = zi.stream_of_frames(c["soff"], len(ORDER))
    gw = c["params"].grid_w
    out = {}
    for f, n in enumerate(ORDER):
        if n in c["planted"]:
            kind, full = rotation[st[f]], hand_count(c["planted"][n], gw, c["R"], 4.0, 2)
            count = full if kind == "all" else None if n not in c["whole"] else full if kind == "own" else 0
            out[f] = (count, hand_rose(c["planted"][n]))
    return out


FLOW_EACH = tuple(range(len(ORDER) + 1))       # one stream per frame: the planted frames' maps stand alone


@functools.lru_cache(maxsize=None)
def flow_expected(name, soff):
    c = lanes_case(name)
    return frozen(lm.flow_map(c["params"], c["mv"], c["off"], c["sd"], np.array(soff, dtype=np.uint64)))[0]


# Plane base phases.  The staged copy moves up to three head bytes, aligned words and up to three tail bytes; what it
# meets is decided by the source's phase inside a 32-bit word, ((s gh + y_lo) gw + shift) % 4 for stream s of a plane
# tensor that starts `shift` bytes behind an allocation's start, and by the copied bytes, R gw.  The runs: the six
# last-staged shapes and tall-65 of the unstaged limit (which copies nothing and reads bytes from memory), each at shifts
# 0 .. 3; the shifts give every shape every phase, and the six staged shapes end on 0, 1 and 2 bytes behind the last
# word.  phase_runs() adds the first staged shape of more than four columns and margin (1 .. 3 rows) with R gw % 4 == 3 —
# found when this was written: wide-staged-6931x3 with a margin of one row, which leaves ONE analysed row between two halo
# rows; no code reads that.  More than four columns: there the last cell of the last analysed row belongs to a corner
# pair of E whose other cell can be a centre, so one wrong byte at the very end of the copy changes a count (on two
# columns nothing is a centre; on three and four the last column's pair is vertical and neither cell can be one).
PHASE_SHIFTS = (0, 1, 2, 3)
PHASE_ROTATION = LANES_ROTATIONS[0]


def phase_pairs(gw, gh, margin=0):
    """{(source phase % 4, copied bytes % 4)} over the three streams and the four shifts."""
    return {(((s * gh + margin) * gw + shift) % 4, ((gh - 2 * margin) * gw) % 4) for s in range(3) for shift in PHASE_SHIFTS}


@functools.lru_cache(maxsize=None)
def phase_runs():
    """[(shape name, margin)]"""
    names = [n for n in shapes("lanes") if "-staged-" in n] + [n for n, (gw, _, kind) in shapes("lanes").items() if kind == "tall" and gw == 65]
    runs = [(n, 0) for n in names]
    tails = {(shapes("lanes")[n][0] * shapes("lanes")[n][1]) % 4 for n in names if "-staged-" in n}
    for want in sorted(set(range(4)) - tails):
        runs.append(next((n, mg) for n in names if "-staged-" in n and shapes("lanes")[n][0] > 4 for mg in (1, 2, 3)
                         if shapes("lanes")[n][1] > 2 * mg and (shapes("lanes")[n][0] * (shapes("lanes")[n][1] - 2 * mg)) % 4 == want))
    return runs
