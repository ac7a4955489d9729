"""Inputs of tests/test_gpu_blob_edges.py and tests/test_blob_edges_host.py: the record-level cases of
tests/derived_edge_inputs.py (head, step boundary and tail; 40-byte records on a shifted base; squares at and beyond 2^32),
taken as they are, for the kernels that stream the records twice — blobs_frames_kernel in its resident and pipe form
(csrc/blobs_kernels.hip), gmc_blobs_frames_kernel with its three streaming call sites (csrc/gmc_blobs_kernels.hip) — and
for gmc_frames_kernel.  What is added here: the pan-moved edge batch, the expected values by hand and by the models
(tests/blobs_model.py, tests/gmc_blobs_inputs.py, derived_soak.gmc_counts_np), and one frame pair whose residual reaches
65 535 + 127 on an axis.  Everything is built once per process and handed out read-only."""
import functools

import numpy as np

import mvtrim_amd as m

import blobs_model as bm
import derived_edge_inputs as dei
import gmc_blobs_inputs as gbi
import gmc_model as gm
from derived_edge_inputs import frozen

EDGE_VN = (3, 4)                            # vectors_needed: cell A (exactly 3 voters) is active at 3 and not at 4
EDGE_THR = 4.0                              # |d|^2 = 5 passes
PAN = (7, -3)                               # dst - src of every still record of the pan-moved batch
MS, Q8 = 16, 128
EDGE_STREAMS = dei.EDGE_STREAMS             # two streams: frames [0, 37) and [37, F)
LONG = dei.STEP40 - 1                       # the shortest of the long test frames is head + 4095 records
N_TEST, N_LONG, N_SHORT = 68, 44, 24


def edge_params(vn):
    p = m.ScanParams.from_config(1920, 1080, mv_threshold_sq=EDGE_THR, vectors_needed=vn)
    assert (p.grid_w, p.grid_h, p.vertical_margin, p.block_shift) == (120, 68, 3, 4)
    return p


def edge_soff():
    F = len(dei.edge_batch()[1]) - 1
    return np.array(list(EDGE_STREAMS) + [F], dtype=np.uint64)


def ones_keeps(p, n=1):
    return np.ones((n, p.grid_h, p.grid_w), dtype=bool)


@functools.lru_cache(maxsize=None)
def pan_batch():
    """dei.edge_batch() with every src moved in place by (-7, +3): every displacement grows by the pan (7, -3), no record
    is added or moved, so frame lengths and the residues of the first records are the edge batch's."""
    mv, off, sd, test, cells, lengths = dei.edge_batch()
    F = len(off) - 1
    moved = gm.shift_src(mv, off, np.full(F, -PAN[0]), np.full(F, -PAN[1]))
    assert moved is not None                                         # inside int16
    return frozen(moved)[0], off, sd


def long_test_frames():
    """The test frames of head + BIG_KINDS records (>= 4095): the still records outnumber the 13 voters there."""
    _, _, _, test, _, lengths = dei.edge_batch()
    return [f for f in test if lengths[f][1] >= LONG]


def edge_hand(vn, frames=None):
    """{"centres", "blobs", "largest", "box"} by hand, for `frames` (default: every frame of the batch) in order: a test
    frame at level 3 holds the pair A + N — 2 centres, one blob of 2, the box around the two cells; at level 4 only N is
    active and has no active neighbour; a filler frame holds at most two voters, one per cell: nothing."""
    _, off, _, test, cells, _ = dei.edge_batch()
    F = len(off) - 1
    out = {k: np.zeros(F, dtype=np.uint32) for k in ("centres", "blobs", "largest")}
    out["box"] = np.full((F, 4), 0xFFFF, dtype=np.uint16)
    if vn == 3:
        for f in test:
            (ax, ay), (nx, ny) = cells[f]
            out["centres"][f], out["blobs"][f], out["largest"][f] = 2, 1, 2
            out["box"][f] = (min(ax, nx), min(ay, ny), max(ax, nx), max(ay, ny))
    if frames is not None:
        out = {k: v[list(frames)] for k, v in out.items()}
    return out


@functools.lru_cache(maxsize=None)
def edge_model(vn, masked=False):
    """blobs_model.model_batch on the edge batch; masked: two streams under all-ones keeps."""
    mv, off, sd = dei.edge_batch()[:3]
    p = edge_params(vn)
    if masked:
        return bm.model_batch(p, mv, off, sd, edge_soff(), ones_keeps(p, 2))
    return bm.model_batch(p, mv, off, sd)


@functools.lru_cache(maxsize=None)
def edge_gmc_model(vn, moved, max_shift, masked=False):
    """gmc_blobs_inputs.model_batch on the edge batch (moved: on the pan-moved one), min_share_q8 128."""
    mv, off, sd = pan_batch() if moved else dei.edge_batch()[:3]
    p = edge_params(vn)
    if masked:
        return gbi.model_batch(p, mv, off, sd, max_shift, Q8, edge_soff(), ones_keeps(p, 2))
    return gbi.model_batch(p, mv, off, sd, max_shift, Q8)


def pipe_frames(moved):
    """The frames of the batch as the pipe is fed them: one record array per frame."""
    mv, off, _ = pan_batch() if moved else dei.edge_batch()[:3]
    return [mv[int(off[f]):int(off[f + 1])] for f in range(len(off) - 1)]


# ------------------------------------------------------------------ 40-byte records on a shifted base

UNALIGNED_KEEP_DENSITY = 0.85
UNALIGNED_SOFF = np.array([0, 13, 40], dtype=np.uint64)
UNALIGNED_SHIFT_SETTINGS = (0, MS)


def unaligned_params():
    return m.ScanParams.from_config(1920, 1080)


@functools.lru_cache(maxsize=None)
def unaligned_keeps(kind):
    """bool [2, 68, 120]: "ones", or "random": each cell kept with probability 0.85, one plane per stream."""
    p = unaligned_params()
    if kind == "ones":
        return frozen(ones_keeps(p, 2))[0]
    return frozen(np.random.RandomState(85).rand(2, p.grid_h, p.grid_w) < UNALIGNED_KEEP_DENSITY)[0]


@functools.lru_cache(maxsize=None)
def unaligned_model(max_shift=None, keep=None):
    """max_shift None: the blob model; else the compensated one (min_share_q8 128).  keep: None, "ones" or "random"."""
    mv, off, sd = dei.unaligned_batch()
    p = unaligned_params()
    soff, keeps = (None, None) if keep is None else (UNALIGNED_SOFF, unaligned_keeps(keep))
    if max_shift is None:
        return bm.model_batch(p, mv, off, sd, soff, keeps)
    return gbi.model_batch(p, mv, off, sd, max_shift, Q8, soff, keeps)


# ------------------------------------------------------------------ squares at and beyond 2^32

BIG_VN = (1, 2)
BIG_BOX = (30, 31, 30, 31)


def big_params(thr, vn):
    p = m.ScanParams.from_config(32768, 32768, mv_threshold_sq=thr, vectors_needed=vn, **dei.BIG_KW)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (32, 32, 0)
    return p


def big_hand(thr, vn):
    """Per frame of dei.big_frames(): the helpers' cell (30, 31) is the only possible centre — (31, 31) lies in the last
    column — so a count of 1 is one blob of one cell with the box (30, 31, 30, 31)."""
    ce = dei.big_hand_count(thr, vn)
    return {"centres": ce, "blobs": ce, "largest": ce, "box": [BIG_BOX if c else bm.NO_BOX for c in ce]}


# The residual's own square: a record that moves by 65 535 on one axis under a pan of -127 on that axis has the residual
# 65 535 + 127 = 65 662, whose square 4 311 498 244 is >= 2^32 where 65 535^2 = 4 294 836 225 is not; cut to 32 bits it
# reads 16 530 948.  At the threshold 2^32 and vectors_needed 2 the cell of the two big records is active iff the pan is
# applied and the square is kept whole, and its neighbour — two helpers, whose magnitude passes with or without the pan —
# is then the frame's one centre.
PAN_BIG_MS, PAN_BIG_THR, PAN_BIG_VN = 127, 4294967296.0, 2
PAN_BIG_FILLERS = 8
R_BIG = 65535 + 127


def _pan_big_frame(axis):
    """axis 0: the pan is (-127, 0); the big pair sits in cell (31, 31) (the last column: never a centre), the helpers in
    (30, 31).  axis 1: the pan is (0, -127); the big pair sits in (10, 31), the helpers in (11, 31).  Eight fillers in
    cell (5, 5) carry the pan."""
    mv = np.zeros(4 + PAN_BIG_FILLERS, dtype=m.MV_DTYPE)
    if axis == 0:
        mv["dst_x"][:4], mv["dst_y"][:4] = [32767, 32767, 31743, 31743], 32767
        mv["src_x"][:4], mv["src_y"][:4] = -32768, [32767, 32767, -32768, -32768]
    else:
        mv["dst_x"][:4], mv["dst_y"][:4] = [10752, 10752, 11776, 11776], 32767
        mv["src_x"][:4], mv["src_y"][:4] = [10752, 10752, -32768, -32768], -32768
    mv["dst_x"][4:], mv["dst_y"][4:] = 5 * 1024 + 512, 5 * 1024 + 512
    mv["src_x"][4:] = mv["dst_x"][4:] + (127 if axis == 0 else 0)
    mv["src_y"][4:] = mv["dst_y"][4:] + (127 if axis == 1 else 0)
    return mv


@functools.lru_cache(maxsize=None)
def pan_big_frames():
    """(mv, off, sd): two frames, the pan on x and the pan on y."""
    b = m.FrameBatch.from_frames([_pan_big_frame(0), _pan_big_frame(1)])
    return frozen(np.ascontiguousarray(b.mv, dtype=m.MV_DTYPE).copy(), np.ascontiguousarray(b.frame_off, dtype=np.uint64),
                  np.ones(2, dtype=np.uint8))


def pan_big_hand(max_shift):
    """(blob outputs, info rows) from exact Python integers.  12 records are counted; 8 move by -127 on the pan's axis
    (share 8 / 12 >= 1 / 2) and 10 by 0 on the other.  With max_shift 127 the pan is applied: the big pair's residual
    square is 65 662^2 >= 2^32, its cell is active, the helpers' cell is a centre.  With max_shift 0 only the bin 0 exists
    (no record on the pan's axis, 10 on the other): nothing is applied, 65 535^2 < 2^32, no centre."""
    assert R_BIG * R_BIG >= 2 ** 32 > 65535 * 65535 and (R_BIG * R_BIG) % 2 ** 32 < 2 ** 32 - 1
    helper = [(64511 + 127) ** 2 + 65535 ** 2, 64511 ** 2 + 65535 ** 2, 44544 ** 2 + (65535 + 127) ** 2, 44544 ** 2 + 65535 ** 2]
    assert min(helper) >= 2 ** 32
    if max_shift == 0:
        blobs = {"centres": [0, 0], "blobs": [0, 0], "largest": [0, 0], "box": [bm.NO_BOX, bm.NO_BOX]}
        return blobs, [(0, 0, 0, 0, 12, 0, 10), (0, 0, 0, 0, 12, 10, 0)]
    # frame 1: column 10 is an inner column, so the big pair's cell is a centre too: one blob of two cells
    blobs = {"centres": [1, 2], "blobs": [1, 1], "largest": [1, 2], "box": [(30, 31, 30, 31), (10, 31, 11, 31)]}
    return blobs, [(-127, 0, -127, 0, 12, 8, 10), (0, -127, 0, -127, 12, 10, 8)]
