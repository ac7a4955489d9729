"""Inputs of tests/test_gpu_gmc_blobs.py and tests/test_gmc_blobs_host.py (the compensated blob scan,
include/mtgpu_gmc_blobs.h), built once per process and handed out read-only, and the model.

The model holds no new arithmetic: pipe_gmc_inputs.estimate (the masked estimate of steps 1 - 4), the residual active
plane of pipe_gmc_inputs.residual_centres — restated here only because that function returns the count, not the plane —
and blobs_model.blob_stats on its centres.

The workhorse is the PAN EMBEDDING, embed(): any batch and a pan (a, b) -> the batch with (a, b) subtracted from every
record's src and, in every frame with side data, strictly more FILLER records than the frame owns, each displaced by
exactly (a, b), in in-bounds cells of the analysed rows and, under a mask, in kept cells.  Then
  - both modes are (a, b), with a share above one half: the fillers alone outnumber every other counted record;
  - a filler's residual is 0, below every threshold >= 1: it votes nowhere;
  - by consequence C the compensated blob scan of the embedded batch equals the plain blob scan of the original on all
    five outputs — the hand values tests/blobs_inputs.py carries already."""
import collections
import functools

import numpy as np

import mvtrim_amd as m
from mvtrim_amd import _abi

import blobs_inputs as bi
import blobs_model as bm
import derived_cliff_inputs as dci
import gmc_model as gm
import pipe_gmc_inputs as pgi
import zones_inputs as zi
from derived_edge_inputs import MI355X_LDS, frozen, voters
from scan_checks import junk_padding

INFO_FIELDS = ("gx", "gy", "mode_x", "mode_y", "n_in", "n_x", "n_y")
MS, Q8 = pgi.MS, pgi.Q8                     # 16, 128: the defaults of the Python layer and the command


# ------------------------------------------------------------------ the model

def residual_plane(p, mv, gx, gy, keep=None):
    """(active bool [gh, gw], analysed rows bool [gh, 1]) of one frame WITH side data: every record inside the bounds votes
    its residual; active = votes >= vn AND (keep OR the row is not analysed).  Line for line the plane inside
    pipe_gmc_inputs.residual_centres."""
    gw, gh, mg = p.grid_w, p.grid_h, p.vertical_margin
    rows = np.zeros((gh, 1), dtype=bool)
    rows[min(mg, gh):max(gh - mg, min(mg, gh))] = True
    votes = np.zeros((gh, gw), dtype=np.int64)
    t = gm.threshold_int(p.mv_threshold_sq)
    if len(mv) and t is not None:
        dx, dy = gm.displacements(mv)
        rx, ry = dx - gx, dy - gy
        cx, cy = gm.cells(p, mv)
        ok = gm.counted(p, mv) & (rx * rx + ry * ry >= t)
        np.add.at(votes, (cy[ok], cx[ok]), 1)
    act = np.minimum(votes, 255) >= (p.vectors_needed & 0xFF)
    if keep is not None:
        act = act & (np.asarray(keep, dtype=bool) | ~rows)
    return act, rows


def centre_plane(p, mv, gx, gy, keep=None):
    """blobs_model.centre_plane on the residual plane."""
    act, rows = residual_plane(p, mv, gx, gy, keep)
    z = np.pad(act, 1)
    nb = z[1:-1, :-2] | z[1:-1, 2:] | z[:-2, 1:-1] | z[2:, 1:-1]
    cen = act & nb & rows
    cen[:, :1] = False
    cen[:, max(p.grid_w - 1, 0):] = False
    return cen


def frame_model(p, mv, max_shift, min_share_q8, keep=None):
    """((centres, blobs, largest, box), info row in the order of INFO_FIELDS) of one frame WITH side data."""
    gx, gy, n_in, mx, nx, my, ny = pgi.estimate(p, mv, max_shift, min_share_q8, keep)
    return bm.blob_stats(centre_plane(p, mv, gx, gy, keep)), (gx, gy, mx, my, n_in, nx, ny)


def model_batch(p, mv, off, sd, max_shift, min_share_q8, soff=None, keeps=None):
    """{"centres", "blobs", "largest": uint32 [F], "box": uint16 [F, 4], "info": int64 [F, 7]} of a batch; keeps: bool
    [S, gh, gw] with soff, or both None.  A frame without side data, and under a mask a frame behind the last stream,
    reads 0, an all-0xFFFF box and a zero info."""
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else np.zeros(F, dtype=np.int64)
    out = {k: np.zeros(F, dtype=np.uint32) for k in ("centres", "blobs", "largest")}
    out["box"] = np.full((F, 4), 0xFFFF, dtype=np.uint16)
    out["info"] = np.zeros((F, 7), dtype=np.int64)
    for f in range(F):
        if not has[f] or (keeps is not None and not 0 <= st[f] < len(keeps)):
            continue
        (c, b, g, box), info = frame_model(p, mv[int(off[f]):int(off[f + 1])], max_shift, min_share_q8,
                                           None if keeps is None else keeps[st[f]])
        out["centres"][f], out["blobs"][f], out["largest"][f], out["box"][f], out["info"][f] = c, b, g, box, info
    return out


def info_rows(info):
    """GMC_INFO_DTYPE [F] -> int64 [F, 7] in the order of INFO_FIELDS."""
    return np.stack([np.asarray(info[k]).astype(np.int64) for k in INFO_FIELDS], axis=1)


# ------------------------------------------------------------------ the pan embedding

Embedded = collections.namedtuple("Embedded", "mv off pan fillers")


def filler_cells(p, keep=None):
    """The cells a filler may sit in: in bounds, on an analysed row and, under a mask, kept — in row-major order."""
    rows = np.zeros((p.grid_h, 1), dtype=bool)
    mg = p.vertical_margin
    rows[min(mg, p.grid_h):max(p.grid_h - mg, min(mg, p.grid_h))] = True
    ok = np.broadcast_to(rows, (p.grid_h, p.grid_w)).copy()
    if keep is not None:
        ok &= np.asarray(keep, dtype=bool)
    ys, xs = np.nonzero(ok)
    return xs, ys


def embed(p, mv, off, sd, pan, soff=None, keeps=None, seed=0):
    """The pan embedding of the module docstring -> Embedded(mv, off, the pan used, fillers per frame), or None where no
    sign of the pan keeps every src inside int16 or a frame with side data has no cell for its fillers.  The sign of each
    axis is chosen per batch: the first of (a, b), (-a, b), (a, -b), (-a, -b) that fits.  A frame behind the last stream
    has no plane: its fillers go anywhere on the analysed rows.  Records are shuffled inside each frame; the fillers get
    junk padding like any record."""
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    st = zi.stream_of_frames(soff, F) if keeps is not None else None
    a0, b0 = pan
    for a, b in ((a0, b0), (-a0, b0), (a0, -b0), (-a0, -b0)):
        sx = mv["src_x"].astype(np.int64) - a
        sy = mv["src_y"].astype(np.int64) - b
        if len(mv) == 0 or (min(sx.min(), sy.min()) >= -32768 and max(sx.max(), sy.max()) <= 32767):
            break
    else:
        return None
    rng = np.random.RandomState(seed)
    half = (1 << p.block_shift) >> 1
    frames, fillers = [], []
    for f in range(F):
        own = np.array(mv[int(off[f]):int(off[f + 1])])
        own["src_x"] = own["src_x"].astype(np.int64) - a
        own["src_y"] = own["src_y"].astype(np.int64) - b
        if not has[f]:
            frames.append(own), fillers.append(0)
            continue
        keep = None
        if keeps is not None and 0 <= st[f] < len(keeps):
            keep = keeps[st[f]]
        xs, ys = filler_cells(p, keep)
        n = len(own) + 1
        if len(xs) == 0:
            return None
        pick = (np.arange(n) + rng.randint(0, len(xs))) % len(xs)
        fill = np.zeros(n, dtype=m.MV_DTYPE)
        fill["dst_x"], fill["dst_y"] = (xs[pick] << p.block_shift) + half, (ys[pick] << p.block_shift) + half
        fsx, fsy = fill["dst_x"].astype(np.int64) - a, fill["dst_y"].astype(np.int64) - b
        if min(fsx.min(), fsy.min()) < -32768 or max(fsx.max(), fsy.max()) > 32767:
            return None
        fill["src_x"], fill["src_y"] = fsx, fsy
        both = np.concatenate([own, junk_padding(fill, rng)])
        frames.append(both[rng.permutation(len(both))]), fillers.append(n)
    counts = np.array([len(fr) for fr in frames], dtype=np.uint64)
    off2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    mv2 = np.concatenate(frames) if frames else np.zeros(0, dtype=m.MV_DTYPE)
    return Embedded(*frozen(np.ascontiguousarray(mv2, dtype=m.MV_DTYPE), off2), (a, b), tuple(fillers))


# the blob cases that run under the embedding: name -> (maker, pan).  Pans differ per case so that both signs, both axes
# and the ends of the default max_shift occur.
REUSED = collections.OrderedDict([
    ("edge_columns", (bi.edge_columns_case, (9, 3))),
    ("halo_row", (bi.halo_row_case, (-7, 2))),
    ("seam-65", (lambda: bi.seam_case(65), (16, -16))),
    ("seam-129", (lambda: bi.seam_case(129), (1, 0))),
    ("seam-130", (lambda: bi.seam_case(130), (0, -5))),
    ("late_merge", (bi.late_merge_case, (-16, 16))),
    ("serpentine-66x12", (lambda: bi.serpentine_case("66x12"), (9, 3))),
    ("serpentine-4k", (lambda: bi.serpentine_case("4k"), (-3, -11))),
    ("spiral", (lambda: bi.serpentine_case("spiral"), (12, 1))),
    ("domino-1080p", (lambda: bi.domino_case("1080p"), (2, -2))),
    ("domino-4k", (lambda: bi.domino_case("4k"), (9, 3))),
    ("everything-6", (lambda: bi.everything_case(6), (5, 5))),
    ("everything-0", (lambda: bi.everything_case(0), (-1, 15))),
    ("tie", (bi.tie_case, (9, 3))),
])


@functools.lru_cache(maxsize=None)
def reused_case(name):
    """(Case, Embedded or None, Embedded without the masks or None).  The second embedding is made only for the masked
    cases that also run without their masks (the word seams)."""
    make, pan = REUSED[name]
    c = make()
    e = embed(c.p, c.mv, c.off, c.sd, pan, c.soff, c.keeps, seed=len(name))
    plain = embed(c.p, c.mv, c.off, c.sd, pan, seed=len(name) + 1) if name.startswith("seam") else None
    return c, e, plain


# ------------------------------------------------------------------ 1. the rule bites: hand frames on the 1080p grid

P4_PAIRS = [(50, 25), (51, 25), (60, 25), (61, 25), (50, 30), (51, 30), (60, 30), (61, 30)]
O8_OBJECT = pgi.block(50, 25, 4, 2)
OVERLAY = pgi.block(5, 6, 10, 3)
OBJECT_D = (14, 3)                           # the objects' own displacement: residual (5, 0) under the pan (9, 3)


def bite_frame(objects, overlay=False):
    """The pan (9, 3) on block(0, 20, 120, 20) minus the object cells, 2 records each; the objects move by (14, 3); the
    overlay, where asked for, is still."""
    groups = [([c for c in pgi.PAN_ROWS if c not in objects], pgi.PAN), (objects, OBJECT_D)]
    if overlay:
        groups.append((OVERLAY, (0, 0)))
    return pgi.cells_frame(groups)


@functools.lru_cache(maxsize=None)
def bite_frames():
    """{name: frame} on the grid of pipe_gmc_inputs (120 x 68, margin 3, vn 2, cn 2, threshold 16).

    P4   four isolated pairs.  Counted: 2400 cells x 2 = 4800 records.  x: the 8 object cells' 16 records move by 14, so
         n_x = 4800 - 16 = 4784 at mode 9; y: every record moves by 3, n_y = 4800.  Both supported (4784 * 256 >= 128 * 4800).
         Residuals: the pan's are 0; the objects' are (5, 0), 25 >= 16, two votes per cell = vn: 8 active cells, each
         with its partner as the only active neighbour: 8 centres in 4 blobs of 2; the first in row-major order is
         (50, 25)-(51, 25): box (50, 25, 51, 25).
    O8   one object block(50, 25, 4, 2): the same 8 cells' worth of records, so the same info; all 8 cells active, every
         one has a neighbour inside the block: 8 centres, 1 blob of 8, box (50, 25, 53, 26).
    P4 + overlay   30 still cells, 60 records, on rows 6 .. 8 (analysed: margin 3).  No mask: n_in 4860, n_x 4784 and n_y
         4800 as before, still supported (4784 * 256 = 1 224 704 >= 128 * 4860 = 622 080); the overlay's residual (-9, -3)
         passes, a 10 x 3 block in columns 5 .. 14: 30 more centres in one more blob: centres 38, blobs 5, largest 30, box
         (5, 6, 14, 8).  Under a keep plane that clears those 30 cells: not counted (n_in 4800) and not active: P4 again.
    The plain blob scan of P4 and of O8: every record passes on its own magnitude (90 and 205), all 2400 cells of rows
    20 .. 39 are active, columns 1 .. 118 are centres: 20 * 118 = 2360 in one blob, box (1, 20, 118, 39)."""
    fr = {"P4": bite_frame(P4_PAIRS), "O8": bite_frame(O8_OBJECT), "P4+overlay": bite_frame(P4_PAIRS, overlay=True),
          "D": np.array(pgi.hand_frames()["d"])}
    rng = np.random.RandomState(13)
    for k in fr:
        fr[k] = junk_padding(fr[k][rng.permutation(len(fr[k]))], rng)
        fr[k].setflags(write=False)
    return fr


BITE_INFO = (9, 3, 9, 3, 4800, 4784, 4800)
# name -> (frame, keep name or None, (centres, blobs, largest, box), info row)
BITE_HAND = [
    ("P4", "P4", None, (8, 4, 2, (50, 25, 51, 25)), BITE_INFO),
    ("O8", "O8", None, (8, 1, 8, (50, 25, 53, 26)), BITE_INFO),
    ("P4+overlay, no mask", "P4+overlay", None, (38, 5, 30, (5, 6, 14, 8)), (9, 3, 9, 3, 4860, 4784, 4800)),
    ("P4+overlay, mask", "P4+overlay", "C", (8, 4, 2, (50, 25, 51, 25)), BITE_INFO),
]
BITE_PLAIN = (2360, 1, 2360, (1, 20, 118, 39))        # the uncompensated blob scan of P4 and of O8
BITE_KEEPS = {"C": pgi.KEEP_C, "D": pgi.KEEP_D, None: None}


def bite_batch(names):
    """(mv, off, sd) of the named frames, one after the other."""
    fr = bite_frames()
    b = m.FrameBatch.from_frames([fr[n] for n in names])
    return frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
                  np.ones(len(names), dtype=np.uint8))


# ------------------------------------------------------------------ 4. per-stream masks

@functools.lru_cache(maxsize=None)
def streams_case():
    """(params, mv, off, sd, soff, keeps): three streams, two distinct planes, two frames behind the last stream.
        stream 0 (frames 0, 1)   all ones:            P4+overlay -> the no-mask values; O8
        stream 1 (frames 2, 3)   the overlay cleared: P4+overlay -> P4's values; frame 3 has no side data
        stream 2 (frame 4)       all ones again:      case D of pipe_gmc_inputs
        frames 5, 6              behind stream_off[3]: the no-blob answer and a zero info, whatever they hold"""
    names = ["P4+overlay", "O8", "P4+overlay", "O8", "D", "P4", "O8"]
    mv, off, _ = bite_batch(names)
    sd = np.array([1, 1, 1, 0, 1, 1, 1], dtype=np.uint8)
    keeps = np.stack([pgi.ONES, pgi.KEEP_C, pgi.ONES])
    return (pgi.params(), mv, off) + frozen(sd, np.array([0, 2, 4, 5], dtype=np.uint64), keeps)


STREAMS_HAND = [(38, 5, 30, (5, 6, 14, 8)), (8, 1, 8, (50, 25, 53, 26)), (8, 4, 2, (50, 25, 51, 25)), (0, 0, 0, bm.NO_BOX),
                None, (0, 0, 0, bm.NO_BOX), (0, 0, 0, bm.NO_BOX)]          # None: case D without its mask, from the model


# ------------------------------------------------------------------ 3. consequences A and B: random batches

RANDOM = list(range(len(zi.RANDOM_CASES)))


# ------------------------------------------------------------------ 6. limits

def lds_by_hand(gw, R):
    """csrc/gmc_blobs_kernels.h: the blob scan's layout (blobs_inputs.lds_by_hand: the tile, R keep rows, one plane of
    R + 2 mask rows, 32 bytes of totals), two histograms of 256 32-bit bins and 32 bytes of result words."""
    return bi.lds_by_hand(gw, R) + 2 * 256 * 4 + 32


def preview_or_none(p, lds=MI355X_LDS):
    try:
        return m.gmc_blobs_preview(p, lds)
    except m.MtgpuError as e:
        if e.code != _abi.MT_ERR_UNSUPPORTED:
            raise
        return None


LIMIT_TALL_GW, LIMIT_WIDE_GH = (3, 65), (1, 3)


@functools.lru_cache(maxsize=None)
def limit_shapes():
    """{name: (gw, gh, kind)}: the last grids mtgpu_gmc_blobs_preview accepts at 163 840 bytes, by bisection over the
    preview as derived_cliff_inputs does it (grid_params: vertical_mask 0, block_shift 1).  Tall: keep staging and centre
    plane over several trips of the workgroup; wide: the init's leftward scan across many words."""
    out = {}
    for gw in LIMIT_TALL_GW:
        gh = dci.largest(lambda h: preview_or_none(dci.grid_params(gw, h)) is not None)
        out[f"tall-{gw}"] = (gw, gh, "tall")
    for gh in LIMIT_WIDE_GH:
        def ok(w):
            p = dci.grid_params(w, gh)
            return dci.creatable(p) and preview_or_none(p) is not None
        out[f"wide-{gh}"] = (dci.largest(ok, 16383), gh, "wide")
    return out


LIMIT_PAN = (7, 3)
LIMIT_KW = dci.CTX_KW                       # vn 2, threshold 4, cn 2: every planted pair and every blob cell with two votes


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(params, original (mv, off, sd, planted), Embedded): the 12-frame batch of derived_cliff_inputs on the shape, under
    the pan embedding."""
    gw, gh, _ = limit_shapes()[name]
    p = dci.grid_params(gw, gh, **LIMIT_KW)
    mv, off, sd, planted = dci.batch(gw, gh)
    return p, (mv, off, sd, planted), embed(p, mv, off, sd, LIMIT_PAN, seed=gw + gh)


FINE_KW = pgi.FINE_KW                       # 3840 x 2160 -> 960 x 540 cells: row-banded, no form


# ------------------------------------------------------------------ 5. plumbing

@functools.lru_cache(maxsize=None)
def plumbing_case():
    """blobs_inputs.plumbing_case under the embedding, without its masks (one of its planes keeps nothing: no cell for a
    filler): frames without side data, a frame with has_sd == 0 that owns records, nine frames of four shapes."""
    c = bi.plumbing_case()
    return c, embed(c.p, c.mv, c.off, c.sd, (9, 3), seed=5)
