"""Inputs of tests/test_gpu_blob_planes.py and tests/test_blob_planes_host.py: random and adversarial CENTRE PLANES for the
three labelling kernels (csrc/blobs_kernels.hip in its resident and its pipe form, csrc/gmc_blobs_kernels.hip; the five
passes of all three are the one text of csrc/blob_label.h), built once per process and handed out read-only.

A plane is a bool [rows, gw] array of ACTIVE cells, a pure function of (gw, rows, seed).  `rows` is the number of
analysed rows of the grid it is made for (grid_h - 2 * margin): batch() puts it on the rows margin .. grid_h - margin - 1,
so a family that promises one blob keeps it under a vertical margin too.  A plane becomes records as
blobs_inputs.cells_frame makes them (one vote of |d|^2 = 25 per active cell, VECTORS_NEEDED 1, CLUSTERS_NEEDED 1;
plane_frame is the same thing without a Python loop per cell), shuffled and with junk padding by blobs_inputs.batch_of.
Expected values are blobs_model.model_batch on those records, never anything read off the plane: which active cell is a
centre (an active neighbour, columns 0 and gw - 1, the margin rows) stays the model's business.

Families
    perc35 .. perc95   rng.rand(rows, gw) < d.  0.6 sits just above the site-percolation threshold (0.5927): hundreds of
                       blobs of every size and one large ragged one, forks and U shapes on every row — unions racing
                       for one root are the norm
    maze               a random spanning tree of the odd lattice (x = 1, 3, .. <= gw - 2; y = 1, 3, .. <= rows - 1) by
                       depth-first search with a random neighbour order, corridors one cell wide: ONE blob whose union
                       order has nothing to do with the row order
    comb_up, comb_down vertical teeth of random length on every second column (1, 3, ..), joined by one full row (columns
                       1 .. gw - 2) at the bottom (teeth up) or at the top (teeth down): every tooth is a tree of its
                       own until one row joins them all, in one pass, from many waves
    bars               every second row full from column 0 to gw - 1 — runs across many 64-bit words, the init's scan to
                       the left — but for 0 .. 3 single-cell gaps; 0 .. 3 single-cell bridges between each pair of
                       neighbouring bars (0: the two stay apart unless something else joins them)
    confetti           non-touching copies of a 3-cell shape (I and L, every orientation) in columns 1 .. gw - 2, placed
                       at random until 40 % of all attempts have failed: every blob has 3 cells, the winner is decided
                       by the tie rule alone (the smallest y * gw + x) and only the box tells a right one from a wrong one
    -lr, -ud           the left-right and the up-down mirror image of perc60, maze and both combs: the same connectivity,
                       another union order, another tie winner.  No metamorphic assertion on the GPU: every plane is
                       compared with the model's answer for that plane

One batch per grid (GRIDS, smallest first): all of its planes as the frames of one stream in the order of
families_of(), with one frame without side data and one frame with side data and no record in the middle.  The wide grid
takes bars and percolation, the tall one perc60, the maze and the combs.  MASKED adds, on 120 x 68 and on 240 x 135 with
margin 6, the same frames twice: stream 0 under an all-ones plane, stream 1 under a plane that clears a random 15 % of
the cells, which cuts blobs apart."""
import collections
import functools

import numpy as np

import mvtrim_amd as m

import blobs_inputs as bi
import blobs_model as bm
import derived_cliff_inputs as dci
import gmc_blobs_inputs as gbi
from derived_edge_inputs import MI355X_LDS, frozen

PERC = collections.OrderedDict([("perc35", 0.35), ("perc50", 0.5), ("perc60", 0.6), ("perc75", 0.75), ("perc95", 0.95)])
FLIPPED = ("perc60", "maze", "comb_up", "comb_down")
MASK_CLEARED = 0.15
PAN, MAX_SHIFT, MIN_SHARE_Q8 = (9, -3), 16, 128          # check 4 of the GPU tier


# ------------------------------------------------------------------ the generators

def percolation(gw, rows, seed, d):
    return frozen(np.random.RandomState(seed).rand(rows, gw) < d)[0]


def maze(gw, rows, seed):
    rng = np.random.RandomState(seed)
    nx, ny = len(range(1, gw - 1, 2)), len(range(1, rows, 2))
    assert nx >= 1 and ny >= 1
    a = np.zeros((rows, gw), dtype=bool)
    seen = np.zeros((ny, nx), dtype=bool)
    i, j = int(rng.randint(nx)), int(rng.randint(ny))
    seen[j, i] = a[2 * j + 1, 2 * i + 1] = True
    stack = [(i, j)]
    steps = ((1, 0), (-1, 0), (0, 1), (0, -1))
    while stack:
        i, j = stack[-1]
        for k in rng.permutation(4):
            di, dj = steps[k]
            ni, nj = i + di, j + dj
            if 0 <= ni < nx and 0 <= nj < ny and not seen[nj, ni]:
                seen[nj, ni] = True
                a[2 * j + 1 + dj, 2 * i + 1 + di] = a[2 * nj + 1, 2 * ni + 1] = True       # the corridor and the node
                stack.append((ni, nj))
                break
        else:
            stack.pop()
    return frozen(a)[0]


def comb(gw, rows, seed, down):
    rng = np.random.RandomState(seed)
    assert rows >= 2 and gw >= 3
    a = np.zeros((rows, gw), dtype=bool)
    for x in range(1, gw - 1, 2):
        n = int(rng.randint(1, rows))                    # 1 .. rows - 1 cells besides the joining row
        a[rows - 1 - n:rows - 1, x] = True
    a[rows - 1, 1:gw - 1] = True
    return frozen(np.ascontiguousarray(a[::-1]) if down else a)[0]


def _apart(xs):
    """The sorted columns of xs without those that touch the one kept before them: single cells stay single."""
    out = []
    for x in sorted(int(v) for v in xs):
        if not out or x - out[-1] >= 2:
            out.append(x)
    return np.array(out, dtype=np.int64)


def bars(gw, rows, seed):
    rng = np.random.RandomState(seed)
    assert gw >= 8
    a = np.zeros((rows, gw), dtype=bool)
    for y in range(0, rows, 2):
        a[y] = True
        a[y, _apart(rng.randint(2, gw - 2, size=rng.randint(0, 4)))] = False
        if y + 2 < rows:
            a[y + 1, _apart(rng.randint(1, gw - 1, size=rng.randint(0, 4)))] = True
    return frozen(a)[0]


CONFETTI_SHAPES = (((0, 0), (1, 0), (2, 0)), ((0, 0), (0, 1), (0, 2)),                    # I
                   ((0, 0), (1, 0), (0, 1)), ((0, 0), (1, 0), (1, 1)), ((0, 0), (0, 1), (1, 1)), ((1, 0), (0, 1), (1, 1)))   # L


def confetti(gw, rows, seed, min_attempts=50):
    rng = np.random.RandomState(seed)
    a = np.zeros((rows, gw), dtype=bool)
    near = np.zeros((rows + 2, gw + 2), dtype=bool)      # a cell or a 4-neighbour of one, with a frame of one cell
    attempts = fails = 0
    while attempts < min_attempts or fails < 0.4 * attempts:
        shape = CONFETTI_SHAPES[int(rng.randint(len(CONFETTI_SHAPES)))]
        w, h = 1 + max(c[0] for c in shape), 1 + max(c[1] for c in shape)
        x0, y0 = int(rng.randint(1, gw - w)), int(rng.randint(0, rows - h + 1))          # columns 1 .. gw - 2
        cells = [(x0 + dx, y0 + dy) for dx, dy in shape]
        attempts += 1
        if any(near[y + 1, x + 1] for x, y in cells):
            fails += 1
            continue
        for x, y in cells:
            a[y, x] = True
            near[y + 1, x + 1] = near[y, x + 1] = near[y + 2, x + 1] = near[y + 1, x] = near[y + 1, x + 2] = True
    return frozen(a)[0]


def base_plane(family, gw, rows, seed):
    if family in PERC:
        return percolation(gw, rows, seed, PERC[family])
    if family == "maze":
        return maze(gw, rows, seed)
    if family in ("comb_up", "comb_down"):
        return comb(gw, rows, seed, family == "comb_down")
    return {"bars": bars, "confetti": confetti}[family](gw, rows, seed)


def plane(name, gw, rows, seed):
    """The plane called `name`: a family, or a family with -lr / -ud for its mirror image."""
    family, _, flip = name.partition("-")
    a = base_plane(family, gw, rows, seed)
    if flip:
        a = frozen(np.ascontiguousarray(a[:, ::-1] if flip == "lr" else a[::-1]))[0]
    return a


def plane_frame(active, shift=4):
    """The records of a plane: blobs_inputs.cells_frame on its active cells in row-major order (one vote per cell, dst in
    the middle of the cell, dst - src = (5, 0)), for cells of 1 << shift pixels."""
    ys, xs = np.nonzero(active)
    mv = np.zeros(len(xs), dtype=m.MV_DTYPE)
    half = (1 << shift) >> 1
    mv["dst_x"], mv["dst_y"] = (xs << shift) + half, (ys << shift) + half
    mv["src_x"], mv["src_y"] = (xs << shift) + half - 5, (ys << shift) + half
    return mv


# ------------------------------------------------------------------ the case table

Grid = collections.namedtuple("Grid", "name gw gh margin kind")        # kind "": 16-pixel cells through blobs_inputs.grid
GRIDS = collections.OrderedDict((g.name, g) for g in [
    Grid("63x12", 63, 12, 0, ""), Grid("64x12", 64, 12, 0, ""),                           # one word
    Grid("65x34", 65, 34, 0, ""), Grid("128x20", 128, 20, 0, ""), Grid("129x20", 129, 20, 0, ""),    # the seam
    Grid("120x68-m3", 120, 68, 3, ""),
    Grid("wide-2000x9", 2000, 9, 0, "wide"),            # W = 32; derived_cliff_inputs.grid_params, two-pixel cells
    Grid("tall-66x400", 66, 400, 0, "tall"),            # the centre plane takes many trips of the 16 waves
    Grid("240x135-m6", 240, 135, 6, ""), Grid("240x135-m0", 240, 135, 0, ""),
])
MASKED = collections.OrderedDict([("120x68-m3-masked", "120x68-m3"), ("240x135-m6-masked", "240x135-m6")])
BATCHES = list(GRIDS) + list(MASKED)                     # every name batch() knows; GPU_ORDER is smallest first
GPU_ORDER = list(GRIDS)[:6] + ["120x68-m3-masked"] + list(GRIDS)[6:] + ["240x135-m6-masked"]
BIG = ("120x68-m3", "wide-2000x9", "tall-66x400", "240x135-m6", "240x135-m0")           # "120 x 68 and larger"


def with_flips(family):
    return [family, family + "-lr", family + "-ud"] if family in FLIPPED else [family]


def families_of(g):
    """The planes of a grid's batch, in frame order (the two frames without a plane come in the middle: batch())."""
    if g.kind == "wide":
        fams = list(PERC) + ["bars"]
    elif g.kind == "tall":
        fams = ["perc60", "maze", "comb_up", "comb_down"]
    else:
        fams = list(PERC) + ["maze", "comb_up", "comb_down", "bars", "confetti"]
    return [n for f in fams for n in with_flips(f)]


# (grid, family) -> seed.  Not listed: 1 + the family's position in FAMILY_ORDER.  A seed is listed where the default
# one misses the regime tests/test_blob_planes_host.py asserts for the family; no plane is left out instead.
FAMILY_ORDER = list(PERC) + ["maze", "comb_up", "comb_down", "bars", "confetti"]
SEEDS = {
    # nine rows make a strip, not a plane: at d = 0.6 its largest blob stays near 300 cells (316 with the default seed);
    # 6 of the seeds 1 .. 699 reach the 500 the host tier asks of the large grids, this one with 699 cells
    ("wide-2000x9", "perc60"): 387,
}


def seed_of(grid_name, family):
    return SEEDS.get((grid_name, family), 1 + FAMILY_ORDER.index(family))


def params_of(g):
    if g.kind:
        return dci.grid_params(g.gw, g.gh, vectors_needed=1, clusters_needed=1)
    return bi.grid(g.gw, g.gh, g.margin)


def grid_plane(g, name):
    """The plane `name` of grid g on the whole grid: bool [gh, gw], nothing on the margin rows."""
    family = name.partition("-")[0]
    a = np.zeros((g.gh, g.gw), dtype=bool)
    a[g.margin:g.gh - g.margin] = plane(name, g.gw, g.gh - 2 * g.margin, seed_of(g.name, family))
    return frozen(a)[0]


Batch = collections.namedtuple("Batch", "name grid p names frame_of mv off sd soff keeps")


@functools.lru_cache(maxsize=None)
def batch(name):
    """Batch(name, Grid, params, plane names, {plane name: frame}, mv, off, sd, soff, keeps).  soff / keeps (bool [2, gh,
    gw]) are None but for the MASKED names, whose frames are the grid's frames twice."""
    g = GRIDS[MASKED.get(name, name)]
    p = params_of(g)
    names = families_of(g)
    frames = [plane_frame(grid_plane(g, n), p.block_shift) for n in names]
    mid = len(frames) // 2
    frames[mid:mid] = [None, np.zeros(0, dtype=m.MV_DTYPE)]
    frame_of = {n: i + (2 if i >= mid else 0) for i, n in enumerate(names)}
    mv, off, sd = bi.batch_of(frames, 1000 + list(GRIDS).index(g.name))
    assert sd.tolist() == [int(i != mid) for i in range(len(frames))]
    if name not in MASKED:
        return Batch(name, g, p, tuple(names), frame_of, mv, off, sd, None, None)
    F = len(frames)
    keeps = np.ones((2, g.gh, g.gw), dtype=bool)
    keeps[1] = np.random.RandomState(2000 + list(GRIDS).index(g.name)).rand(g.gh, g.gw) >= MASK_CLEARED
    off2 = np.concatenate([off, off[1:] + off[-1]]).astype(np.uint64)
    mv2 = np.tile(mv.view(np.uint8), 2).view(m.MV_DTYPE)     # byte for byte, junk padding included (np.concatenate packs the dtype)
    return Batch(name, g, p, tuple(names), frame_of, *frozen(mv2, off2, np.concatenate([sd, sd]),
                                                             np.array([0, F, 2 * F], dtype=np.uint64), keeps))


@functools.lru_cache(maxsize=None)
def expected(name):
    """blobs_model.model_batch of the batch, read-only.  A MASKED batch: its first stream runs under an all-ones plane on
    the very records of the grid's own batch, so those frames read expected(grid) (the host tier holds that to the model
    under the all-ones plane); only the second stream is labelled again."""
    b = batch(name)
    if name in MASKED:
        F = len(b.sd) // 2
        first = expected(b.grid.name)
        second = bm.model_batch(b.p, b.mv, b.off[F:], b.sd[F:], np.array([0, F], dtype=np.uint64), b.keeps[1:])
        out = {k: np.concatenate([first[k], second[k]]) for k in first}
    else:
        out = bm.model_batch(b.p, b.mv, b.off, b.sd)
    frozen(*out.values())
    return out


@functools.lru_cache(maxsize=None)
def embedded(name):
    """gmc_blobs_inputs.embed of the batch under PAN, or None."""
    b = batch(name)
    return gbi.embed(b.p, b.mv, b.off, b.sd, PAN, b.soff, b.keeps, seed=BATCHES.index(name))


@functools.lru_cache(maxsize=None)
def expected_embedded(name):
    """gmc_blobs_inputs.model_batch of the embedded batch (all six outputs), read-only."""
    b, e = batch(name), embedded(name)
    out = gbi.model_batch(b.p, e.mv, e.off, b.sd, MAX_SHIFT, MIN_SHARE_Q8, b.soff, b.keeps)
    frozen(*out.values())
    return out


def stats(name, plane_name, want=None):
    """(centres, blobs, largest, box) of a plane's frame in the model's answer for the batch."""
    want = expected(name) if want is None else want
    f = batch(name).frame_of[plane_name]
    return int(want["centres"][f]), int(want["blobs"][f]), int(want["largest"][f]), tuple(int(v) for v in want["box"][f])


def pipe_frames(b, lo=0, hi=None):
    """The frames lo .. hi - 1 of a batch as ScanPipe.feed takes them: None without side data, else the record array."""
    hi = len(b.sd) if hi is None else hi
    return [b.mv[int(b.off[f]):int(b.off[f + 1])] if b.sd[f] else None for f in range(lo, hi)]


def preview_lds(p):
    return m.blobs_preview(p, MI355X_LDS)["lds_bytes"], m.gmc_blobs_preview(p, MI355X_LDS)["lds_bytes"]
