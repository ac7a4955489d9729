"""Inputs of tests/test_pipe_persist_host.py and tests/test_gpu_pipe_persist.py (the largest blob's box through the pipe,
include/mtgpu_pipe_boxes.h, and persistence on the decode path), built once and frozen.  Every expected value comes from
tests/blobs_model.py (the flood fill, boxes included), tests/persist_model.py (the rule) or is spelled out by hand in the
docstring of its case; nothing here comes from the GPU."""
import functools

import numpy as np

import mvtrim_amd as m

import blobs_model as bm
import persist_model as pm
import pipe_blobs_inputs as pb
from blobs_inputs import cells_frame, grid
from pipe_blobs_inputs import BIG, BLOCK, GH, GW, LONE, PAIRS, block, freeze

NO_BOX = bm.NO_BOX
MAX_FRAMES = 5                      # frames per batch in the box tests: every input below takes at least three batches

# Two blobs of 6 cells each.  The winner is the blob that holds the smallest y * gw + x.
TIE_LEFT_FIRST = block(20, 10, 3, 2) + block(80, 40, 3, 2)      # the upper one is also the left one: box (20, 10, 22, 11)
TIE_RIGHT_FIRST = block(80, 10, 3, 2) + block(20, 40, 3, 2)     # the upper one is the right one: box (80, 10, 82, 11)
TALL = block(50, 0, 2, GH)                                       # two columns over every row of the grid


@functools.lru_cache(maxsize=None)
def all_frames():
    """23 frames: the 14 of pipe_blobs_inputs.shapes_case (frames without side data first, in the middle and last, a frame
    with side data and no record, ragged frames, a run across the column-63/64 word seam), the 4 of seam_case (runs that
    touch only at the seam, and frame 3: two blobs of 4 — a tie), the 2 of mask_case, the two ties above and TALL, whose
    blob touches the first and the last analysed row of whatever band the parameters analyse."""
    frames = list(pb.shapes_case()[1]) + list(pb.seam_case()[1]) + list(pb.mask_case()[1])
    frames += [cells_frame(TIE_LEFT_FIRST), cells_frame(TIE_RIGHT_FIRST), cells_frame(TALL)]
    assert len(frames) == 23
    return freeze(frames)


@functools.lru_cache(maxsize=None)
def settings():
    """name -> (params, min_blob_cells): CLUSTERS_NEEDED 8 with 3 cells (quiet frames, frames the blob rule drops), 1 with
    1 cell (every frame with a centre is flagged: every box is specified), and the 1080p grid with its margin of 3 rows at
    2 cells (boxes offset by the band's first row: TALL reads rows 3 .. 64)."""
    pm3 = m.ScanParams.from_config(1920, 1080, vectors_needed=1, clusters_needed=1)
    assert (pm3.grid_w, pm3.grid_h, pm3.vertical_margin) == (GW, GH, 3)
    return {"cn8": (grid(GW, GH, 0, vn=1, cn=8), 3), "cn1": (grid(GW, GH, 0, vn=1, cn=1), 1), "margin3": (pm3, 2)}


def keep_plane():
    """pipe_blobs_inputs.mask_case's mask: columns 42 and 82 cleared on every row."""
    return pb.mask_case()[2]


@functools.lru_cache(maxsize=None)
def expected(name, masked):
    """{"flags", "centres", "largest": lists, "box": list of 4-tuples} of all_frames() under settings()[name], by the
    flood-fill model; the box is NO_BOX wherever the flag is 0 (what ScanPipe.drain_boxes hands out)."""
    p, mb = settings()[name]
    mv, off, sd = pb.batch_arrays(all_frames())
    if masked:
        out = bm.model_batch(p, mv, off, sd, np.array([0, len(all_frames())], dtype=np.uint64), np.asarray(keep_plane(), dtype=bool)[None])
    else:
        out = bm.model_batch(p, mv, off, sd)
    flags = bm.flags_np(p, out["centres"], out["largest"], mb).tolist()
    box = [tuple(int(v) for v in b) if fl else NO_BOX for b, fl in zip(out["box"].tolist(), flags)]
    return {"flags": flags, "centres": out["centres"].tolist(), "largest": out["largest"].tolist(), "box": box,
            "model_box": [tuple(int(v) for v in b) for b in out["box"].tolist()]}


# ------------------------------------------------------------------ a reused pinned block

@functools.lru_cache(maxsize=None)
def stale_case():
    """(params, min_blob_cells, batch 1, batch 2, boxes 1, flags 2, boxes 2) at CLUSTERS_NEEDED 8, 3 cells.
    Batch 1: the block of 3 x 4 at (20, 12) three times and the block of 2 x 4 at (40, 30): four flagged frames.
    Batch 2, into the same slots: a block of 3 x 4 at (80, 40) (flag 1, another box), one lone cell (no centre: the early
    exit, which stores no box), no side data (the planner, which stores no box), the block of 3 x 4 at (20, 12)."""
    p = grid(GW, GH, 0, vn=1, cn=8)
    one = [cells_frame(BIG), cells_frame(BIG), cells_frame(BIG), cells_frame(BLOCK)]
    two = [cells_frame(block(80, 40, 4, 3)), cells_frame(LONE), None, cells_frame(BIG)]
    b1 = [(20, 12, 23, 14)] * 3 + [(40, 30, 43, 31)]
    b2 = [(80, 40, 83, 42), NO_BOX, NO_BOX, (20, 12, 23, 14)]
    return p, 3, freeze(one), freeze(two), b1, [1, 0, 0, 1], b2


# ------------------------------------------------------------------ the seams: a hand-made recording of 40 frames at 10 fps

SEAM_FPS, SEAM_FRAMES = 10.0, 40
SEAM_KEYS = (0, 20, 30)                           # key frames: no side data
SEAM_M = (8, 9, 10, 19, 21, 22, 33)               # motion frames: 8 .. 10; 19, 21, 22 around the key frame 20; 33 alone
SEAM_KEPT = (8, 9, 10, 19, 21, 22)                # at MIN_RUN 3


def seam_classes(extra_quiet=()):
    """(flags, has_sd) of the recording; extra_quiet: M frames turned into Q frames."""
    fl = np.zeros(SEAM_FRAMES, dtype=np.uint8)
    sd = np.ones(SEAM_FRAMES, dtype=np.uint8)
    fl[[f for f in SEAM_M if f not in extra_quiet]] = 1
    sd[list(SEAM_KEYS)] = 0
    return fl, sd


def seam_frames(extra_quiet=()):
    """The recording's frames: the block of 2 x 4 (8 centres, one blob) on the M frames, one lone cell (votes, no centre)
    on the quiet ones, None on the key frames."""
    fl, sd = seam_classes(extra_quiet)
    return freeze([None if not sd[f] else cells_frame(BLOCK) if fl[f] else cells_frame(LONE) for f in range(SEAM_FRAMES)])


def seam_pts():
    """pts as the host layer computes them from a .mtmv with time base 1 / 10: frame->pts * av_q2d(time_base)."""
    return [float(f) * (1.0 / SEAM_FPS) for f in range(SEAM_FRAMES)]


def seam_expected(min_run, max_dropout, extra_quiet=()):
    """The frames the rule keeps, by the model: one stream, has_sd given, no boxes."""
    fl, sd = seam_classes(extra_quiet)
    out = pm.persist(fl, [0, SEAM_FRAMES], has_sd=sd, box=None, min_run=min_run, max_dropout=max_dropout)
    return [f for f in range(SEAM_FRAMES) if out["flags"][f]], out["run"].tolist()


# ------------------------------------------------------------------ examples/pipe_boxes_example.c, frame for frame

EX_FRAMES, EX_FPS, EX_MIN_BLOB, EX_MIN_RUN, EX_REACH = 300, 30.0, 3, 3, 2


def example_case():
    """(params, frames, pts): the example's recording — a key frame every 30; frames 60 .. 149 one blob of 4 x 2 cells at
    (10 + 35 (f % 3), 10 + 20 (f % 3)); frames 200 .. 259 one at (20 + f - 200, 30); 8 records a frame, dst = 16 g + 8,
    src = dst - (6, 0)."""
    p = m.ScanParams.from_config(1920, 1080, vectors_needed=1, clusters_needed=8)
    frames = []
    for f in range(EX_FRAMES):
        if f % 30 == 0:
            frames.append(None)
            continue
        rain, obj = 60 <= f < 150, 200 <= f < 260
        mv = np.zeros(8 if (rain or obj) else 0, dtype=m.MV_DTYPE)
        if rain or obj:
            gx0, gy0 = (10 + 35 * (f % 3), 10 + 20 * (f % 3)) if rain else (20 + (f - 200), 30)
            k = np.arange(8)
            mv["dst_x"], mv["dst_y"] = 16 * (gx0 + k % 4) + 8, 16 * (gy0 + k // 4) + 8
            mv["src_x"], mv["src_y"] = mv["dst_x"] - 6, mv["dst_y"]
        frames.append(mv)
    return p, freeze(frames), [f / EX_FPS for f in range(EX_FRAMES)]


def example_expected():
    """[(kept frames without boxes), (kept frames with boxes at reach 2)] by the blob model and the persistence model."""
    p, frames, _ = example_case()
    mv, off, sd = pb.batch_arrays(frames)
    st = bm.model_batch(p, mv, off, sd)
    flags = bm.flags_np(p, st["centres"], st["largest"], EX_MIN_BLOB)
    out = []
    for box in (None, st["box"]):
        r = pm.persist(flags, [0, EX_FRAMES], has_sd=sd, box=box, min_run=EX_MIN_RUN, max_dropout=0, reach=EX_REACH)
        out.append([f for f in range(EX_FRAMES) if r["flags"][f]])
    return out
