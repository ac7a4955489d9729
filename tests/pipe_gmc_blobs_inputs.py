"""Inputs of tests/test_gpu_pipe_gmc_blobs.py and tests/test_pipe_gmc_blobs_host.py (the compensated blob scan carried
through the pipe, include/mtgpu_pipe_gmc_blobs.h), built once per process and handed out read-only.

Nothing here holds arithmetic of its own.  The model is gmc_blobs_inputs.frame_model / model_batch (the masked estimate
of pipe_gmc_inputs and the flood fill of blobs_model); the cases are those of gmc_blobs_inputs, pipe_gmc_inputs and
pipe_blobs_inputs.  What is added is the function that turns a model row into what a pair pipe reports — (flag at
min_blob_cells, the ONE count under `report`) — and the slicing of a batch into the frames a pipe is fed.

Every 40-byte frame is made by ONE constructor call on m.MV_DTYPE and its item size is asserted: np.concatenate of
structured arrays drops the record's padding."""
import functools

import numpy as np

import mvtrim_amd as m

import gmc_blobs_inputs as gbi
import pipe_blobs_inputs as pbi
import pipe_gmc_inputs as pgi
import zones_inputs as zi
from derived_edge_inputs import frozen

REPORTS = ("centres", "largest", "vector")
MS, Q8 = pgi.MS, pgi.Q8
MIN_BLOB = 3                                 # the pair's min_blob_cells of case 1


# ------------------------------------------------------------------ model row -> what the pipe reports

def answer(p, stats, info, min_blob_cells, report):
    """(flag, count) of one frame WITH side data from its model row: stats = (centres, blobs, largest, box), info in the
    order of gmc_blobs_inputs.INFO_FIELDS.  flag = centres >= max(1, CLUSTERS_NEEDED) AND largest >= min_blob_cells; the
    count is the centres, the largest blob, or (uint16)gx | (uint16)gy << 16."""
    c, _, g, _ = stats
    flag = int(int(c) >= max(1, p.clusters_needed) and int(g) >= int(min_blob_cells))
    count = {"centres": int(c), "largest": int(g), "vector": pgi.pack_vector(info[0], info[1])}[report]
    return flag, count


def rows(p, frames, max_shift, min_share_q8, keep=None):
    """The model row (stats, info) of every frame, None for a frame without side data."""
    return [None if f is None else gbi.frame_model(p, f, max_shift, min_share_q8, keep) for f in frames]


def answers(p, model_rows, min_blob_cells, report):
    """(flags, counts) lists of a pair pipe from rows(); a frame without side data reads 0, 0 under every report (Q5)."""
    out = [(0, 0) if r is None else answer(p, r[0], r[1], min_blob_cells, report) for r in model_rows]
    return [a for a, _ in out], [b for _, b in out]


def model(p, frames, min_blob_cells, max_shift, min_share_q8, report, keep=None):
    return answers(p, rows(p, frames, max_shift, min_share_q8, keep), min_blob_cells, report)


def batch_answers(p, out, has, min_blob_cells, report):
    """(flags, counts) from a gmc_blobs_inputs.model_batch dict (or the resident call's arrays, info as int64 [F, 7] rows)."""
    fl, co = [], []
    for f in range(len(has)):
        if not has[f]:
            fl.append(0), co.append(0)
            continue
        a = answer(p, (out["centres"][f], out["blobs"][f], out["largest"][f], None), out["info"][f], min_blob_cells, report)
        fl.append(a[0]), co.append(a[1])
    return fl, co


def frame(mv, a, b):
    """Records [a, b) of a batch as a frame of its own: one constructor call, 40-byte items."""
    f = np.array(mv[int(a):int(b)], dtype=m.MV_DTYPE)
    assert f.dtype == m.MV_DTYPE and f.dtype.itemsize == 40 and f.strides == (40,)
    f.setflags(write=False)
    return f


def frames_of(mv, off, sd):
    """A batch -> the tuple of frames a pipe is fed: None where the frame has no side data (its records, if it owns
    any, are not fed: the scan does not read them either)."""
    has = zi.has_side_data(off, sd)
    return tuple(frame(mv, off[f], off[f + 1]) if has[f] else None for f in range(len(off) - 1))


# ------------------------------------------------------------------ 1. the rule bites

# name -> (frame of gmc_blobs_inputs.bite_frames, keep name, flag at MIN_BLOB, centres, largest, vector): BITE_HAND read at
# min_blob_cells 3 and CLUSTERS_NEEDED 2
BITE = [
    ("P4", "P4", None, 0, 8, 2, (9, 3)),
    ("O8", "O8", None, 1, 8, 8, (9, 3)),
    ("P4+overlay, no mask", "P4+overlay", None, 1, 38, 30, (9, 3)),
    ("P4+overlay, mask", "P4+overlay", "C", 0, 8, 2, (9, 3)),
]
BITE_GMC_ALONE = (1, 8)                      # set_gmc on P4 and on O8: 8 centres >= 2
BITE_BLOBS_ALONE = (1, 2360, 2360)           # set_blobs(3) on P4 and on O8: one blob of 2360 (BITE_PLAIN)


def bite_count(row, report):
    _, _, _, _, c, g, vec = row
    return {"centres": c, "largest": g, "vector": pgi.pack_vector(*vec)}[report]


# ------------------------------------------------------------------ 3. both exits write

STALE_PAN = (4, -2)


@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, batch 1, batch 2, batch 3, hand) at (16, 128), min_blob_cells 3, no mask.
    Batch 1: three frames O8: flag 1, centres 8, largest 8, vector (9, 3) — the labelled exit.
    Batch 2: three frames of a pan (4, -2) on rows 20 .. 39 and nothing else: 4800 counted records, all of them in the
    mode, every residual 0: no vote, no centre — the early exit: flag 0, centres 0, largest 0, vector (4, -2), NOT batch
    1's (9, 3).
    Batch 3: three frames without side data — the planning kernel: 0, 0 under every report."""
    o8 = gbi.bite_frames()["O8"]
    quiet = pgi.cells_frame([(pgi.PAN_ROWS, STALE_PAN)])
    assert quiet.dtype == m.MV_DTYPE and quiet.dtype.itemsize == 40 and len(quiet) == 4800
    quiet.setflags(write=False)
    v1, v2 = pgi.pack_vector(9, 3), pgi.pack_vector(*STALE_PAN)
    hand = [{"flags": [1] * 3, "centres": [8] * 3, "largest": [8] * 3, "vector": [v1] * 3},
            {"flags": [0] * 3, "centres": [0] * 3, "largest": [0] * 3, "vector": [v2] * 3},
            {"flags": [0] * 3, "centres": [0] * 3, "largest": [0] * 3, "vector": [0] * 3}]
    return pgi.params(), (o8,) * 3, (quiet,) * 3, (None,) * 3, hand


# ------------------------------------------------------------------ 4. word seams and VECTORS_NEEDED = 0

SEAM_PAN = (9, 3)


@functools.lru_cache(maxsize=None)
def seam_case():
    """(params, frames plain, frames masked, keep, hand): pipe_blobs_inputs.seam_case — blobs across columns 63 | 64 —
    under the pan embedding, without a mask (by consequence C of mtgpu_gmc_blobs.h the hand values of the case) and under
    a keep plane that clears column 63 on every row (the model; the fillers of that embedding sit in kept cells)."""
    p, frames, hand = pbi.seam_case()
    mv, off, sd = pbi.batch_arrays(frames)
    keep = np.ones((pbi.GH, pbi.GW), dtype=bool)
    keep[:, 63] = False
    frozen(keep)
    plain = gbi.embed(p, mv, off, sd, SEAM_PAN, seed=41)
    soff = np.array([0, len(frames)], dtype=np.uint64)
    masked = gbi.embed(p, mv, off, sd, SEAM_PAN, soff, keep[None], seed=42)
    assert plain is not None and masked is not None
    return p, frames_of(plain.mv, plain.off, sd), frames_of(masked.mv, masked.off, sd), keep, hand


@functools.lru_cache(maxsize=None)
def vn0_case():
    """(params, frames, keep): pipe_blobs_inputs.vn0_case — VECTORS_NEEDED 0, one frame with side data and no record —
    under a mask that clears column 64 and row 30: every kept cell is active without a vote.  Expected: the model."""
    p, frames, _ = pbi.vn0_case()
    keep = np.ones((pbi.GH, pbi.GW), dtype=bool)
    keep[:, 64] = False
    keep[30, :] = False
    frozen(keep)
    return p, frames, keep


# ------------------------------------------------------------------ 5. random batches

@functools.lru_cache(maxsize=None)
def random_case(i):
    """(params, frames, keep, has, model unmasked, model masked) of zones_inputs.random_case(i): the pipe has ONE plane, so
    plane 0 of the case serves every frame — one stream that covers the batch.  Settings (16, 64)."""
    p, mv, off, sd, _, keeps = zi.random_case(i)
    F = len(off) - 1
    has = zi.has_side_data(off, sd)
    plain = gbi.model_batch(p, mv, off, sd, MS, 64)
    masked = gbi.model_batch(p, mv, off, sd, MS, 64, np.array([0, F], dtype=np.uint64), keeps[:1])
    return p, frames_of(mv, off, sd), keeps[0], has, plain, masked


# ------------------------------------------------------------------ 6. limits

@functools.lru_cache(maxsize=None)
def limit_frames(name):
    """(params, frames, has, model) of gmc_blobs_inputs.limit_case(name)."""
    p, (_, _, sd, _), e = gbi.limit_case(name)
    assert e is not None
    return p, frames_of(e.mv, e.off, sd), zi.has_side_data(e.off, sd), gbi.model_batch(p, e.mv, e.off, sd, MS, Q8)


@functools.lru_cache(maxsize=None)
def uhd_case():
    """(params, frames[8], hand row): the eight serpentine frames of the 4K grid under their pan embedding: one blob of
    14 817 cells in every frame, one workgroup per CU."""
    c, e, _ = gbi.reused_case("serpentine-4k")
    assert e is not None and len(e.off) - 1 == 8
    return c.p, frames_of(e.mv, e.off, c.sd), (c.hand["centres"][0], c.hand["largest"][0], e.pan)
