"""A flags-only scan of 40-byte records on a single 32-bit tile stops reading a frame once a vote pair proves its flag
(scan_kernels.hip: `vote` under ScanK::early, the poll in stream_mv40).  The proof: the vote that makes a cell active finds
an active 4-neighbour, and BOTH cells lie in columns [1, gw - 2] — the reference's cluster loop (src/motion_scanner.cpp:280)
never visits column 0 or gw - 1, so a pair that touches an edge column holds one centre or none and proves nothing.

Every case compares three results frame for frame: the flags with the exit on, the flags of a context created under
MTGPU_EARLY_EXIT=0, and the C oracle's; the plan key `early_exit` says whether a context takes the exit.  The centre-count
entry point (which never takes it) must return the oracle's exact counts on the same batches.  (The key is read through
mvtrim_amd.early_exit: the keys of MotionScanner.plan are a recorded surface.)  By default only launches of at least
eight frames per CU take the exit; the batches here are a few dozen frames, so their exit-on contexts are created under
MTGPU_EARLY_EXIT=2 (any launch size).  One timing case, with no knob set, shows that the bytes are really skipped.

1080p grid (120 x 68 cells of 16 pixels, analysed rows 3 .. 64 with the default mask) unless a case says otherwise."""
import functools

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import early_exit

import oracle_binding as ob
from scan_checks import device_centres_of, junk_padding, to_device

pytestmark = pytest.mark.gpu

STEP = 4 * 512                     # records of one streaming step: 4 loads in flight per lane, 512 lanes
GW, GH = 120, 68


def params_of(width=1920, height=1080, **kw):
    return ob.params_from_config(width, height, **kw)


def scanners(factory, monkeypatch, p, expect_on, any_size=True, **env):
    """(exit on, exit off) contexts for `p`; `env`: knobs both are created under.  The plan key is asserted.
    any_size: the `on` context is created under MTGPU_EARLY_EXIT=2 — by default the exit is taken by launches of at
    least eight frames per CU, and the batches here hold a few dozen frames (plan key 2; 1 without it)."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.delenv("MTGPU_EARLY_EXIT", raising=False)
    if any_size:
        monkeypatch.setenv("MTGPU_EARLY_EXIT", "2")
    on = factory(p)
    monkeypatch.setenv("MTGPU_EARLY_EXIT", "0")
    off = factory(p)
    monkeypatch.delenv("MTGPU_EARLY_EXIT")
    for k in env:
        monkeypatch.delenv(k)
    assert early_exit.plan(on)["early_exit"] == ((2 if any_size else 1) if expect_on else 0), early_exit.plan(on)
    assert early_exit.plan(off)["early_exit"] == 0, early_exit.plan(off)
    return on, off


def still(n, rng, width=1920, height=1080):
    """n records at rest, anywhere in the frame."""
    mv = np.zeros(n, dtype=m.MV_DTYPE)
    mv["dst_x"] = rng.randint(0, width, size=n)
    mv["dst_y"] = rng.randint(0, height, size=n)
    mv["src_x"], mv["src_y"] = mv["dst_x"], mv["dst_y"]
    return mv


def plant(mv, at, cells, block=16):
    """Records at, at + 1, ... of the frame vote (|d|^2 = 49) for cells[0], cells[1], ... in that order."""
    for i, (cx, cy) in enumerate(cells):
        mv["dst_x"][at + i] = cx * block + (3 * i) % block
        mv["dst_y"][at + i] = cy * block + (5 * i) % block
        mv["src_x"][at + i] = mv["dst_x"][at + i] - 7
        mv["src_y"][at + i] = mv["dst_y"][at + i]
    return mv


def pair_votes(a, b, v, order=0):
    """v votes for each of the cells a and b: alternating (order 0), a's first (1), b's first (2)."""
    if order == 0:
        return [a, b] * v
    return [a] * v + [b] * v if order == 1 else [b] * v + [a] * v


def batch_of(frames, sd=None):
    counts = np.array([len(f) for f in frames], dtype=np.uint64)
    off = np.zeros(len(frames) + 1, dtype=np.uint64)
    np.cumsum(counts, out=off[1:])
    mv = np.concatenate(frames) if frames else np.zeros(0, dtype=m.MV_DTYPE)
    sd = np.ones(len(frames), dtype=np.uint8) if sd is None else np.asarray(sd, dtype=np.uint8)
    return mv, off, sd


def head_records(off):
    """Records of each frame that stream_mv40 hands to lanes 0 .. h-1 ahead of the line-aligned stream, for a batch
    whose base lies on a 128-byte line: 40 h = -start (mod 128)."""
    r = (40 * off[:-1].astype(np.int64)) % 128
    return (13 * ((16 - (r >> 3)) & 15)) & 15


def three_way(on, off_, p, mv, off, sd, what, pinned=False):
    """Flags with the exit on, with it off, and the oracle's, through the device entry point (and the host entry point
    of the `on` context); the centre-count entry point of the `on` context against the oracle's counts."""
    import torch
    want_f, want_c = ob.scan_centres(p, mv, off, sd)
    d_rec, d_off, d_sd = to_device(mv, off, sd, compact=False)
    assert d_rec.data_ptr() % 128 == 0
    n = len(sd)
    got = []
    for s in (on, off_):
        if pinned:
            flags = torch.full((n,), 9, dtype=torch.uint8).pin_memory()
        else:
            flags = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        s.check_frames_device(d_rec, d_off, d_sd, flags)
        torch.cuda.synchronize()
        got.append(flags.cpu().numpy().copy())
    bad = np.flatnonzero((got[0] != want_f) | (got[1] != want_f))
    assert bad.size == 0, (what, bad[:8].tolist(), "want", want_f[bad[:8]].tolist(), "on", got[0][bad[:8]].tolist(),
                           "off", got[1][bad[:8]].tolist(), on.plan)
    host = on.check_frames(m.FrameBatch(mv, off, None, sd))
    assert np.array_equal(host, want_f), (what, "host entry", np.flatnonzero(host != want_f)[:8].tolist())
    fl, ce = device_centres_of(on, d_rec, d_off, d_sd, compact=False)
    assert np.array_equal(ce, want_c.astype(np.uint32)) and np.array_equal(fl, want_f), (what, "centre counts")
    return want_f, want_c


# ------------------------------------------------------------------ where the proving vote sits

@functools.lru_cache(maxsize=None)
def positions_batch(v):
    """Frames whose deciding pair, (50, 30) + (51, 30) with v votes each, ends — the proving vote — in the head records,
    in the first / a middle / the last full step, in the rest behind the last full step and at the very last record;
    each kind after fillers of 0 .. 15 records so that the frames start at every phase of a 128-byte line; each decided
    frame is followed by a still one and by one with a single active cell.  Then frames of the sizes around a
    streaming step, the pair at their end, frames without side data among them."""
    rng = np.random.RandomState(3300 + v)
    a, b = (50, 30), (51, 30)
    frames, sd, kind = [], [], []

    def add(f, has=1, k=""):
        frames.append(junk_padding(f, rng)); sd.append(has); kind.append(k)

    n_main = 3 * STEP + 700
    for phase in range(16):
        add(still(phase, rng), k="filler")
        add(plant(still(n_main, rng), 0, pair_votes(a, b, v, phase % 3)), k="head")
        add(still(n_main - phase, rng), k="still")
        add(plant(still(n_main, rng), 16 + STEP // 2, pair_votes(a, b, v, phase % 3)), k="step0")
        add(plant(still(n_main, rng), 40, [a] * (v + 3)), k="one cell")
        add(plant(still(n_main, rng), 16 + STEP + 2 * STEP // 3, pair_votes(a, b, v, phase % 3)), k="step1")
        add(plant(still(n_main + phase, rng), 15 + 3 * STEP - 2 * v, pair_votes(a, b, v, phase % 3)), k="step2")
        add(plant(still(n_main, rng), n_main - 300, pair_votes(a, b, v, phase % 3)), k="rest")
        add(plant(still(n_main + 3 * phase, rng), n_main + 3 * phase - 2 * v, pair_votes(a, b, v, phase % 3)), k="last")
    for n in (0, 1, 15, 16, 17, STEP - 1, STEP, STEP + 1):
        for has in (1, 1, 0):
            f = still(n, rng)
            if n >= 2 * v:
                plant(f, n - 2 * v, pair_votes(a, b, v))
            add(f, has, k="size")
            add(still(n, rng), k="still")
    mv, off, sd = batch_of(frames, sd)
    for x in (mv, off):
        x.setflags(write=False)
    return mv, off, sd, kind


@pytest.mark.parametrize("v", [1, 2, 4, 7])
def test_proving_vote_in_every_part_of_the_stream(gpu_scanner_factory, monkeypatch, v):
    p = params_of(vectors_needed=v)
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    mv, off, sd, kind = positions_batch(v)
    h = head_records(off)
    heads = [i for i, k in enumerate(kind) if k == "head"]
    # the pair's 2 v votes lie inside the head records of some frames (and beyond them in others) at every v
    assert any(h[i] >= 2 * v for i in heads) and any(h[i] < 2 * v for i in heads), h[heads]
    assert len(set(h[heads].tolist())) >= 8
    want_f, _ = three_way(on, off_, p, mv, off, sd, f"positions, vectors_needed {v}")
    for i, k in enumerate(kind):
        if k in ("head", "step0", "step1", "step2", "rest", "last"):
            assert want_f[i] == 1, (i, k)
        if k in ("still", "filler", "one cell"):
            assert want_f[i] == 0, (i, k)


# ------------------------------------------------------------------ which pairs prove anything

def geometry_frames(v, cases, rng, n=STEP + 300, block=16, width=1920, height=1080):
    frames = []
    for i, cells in enumerate(cases):
        votes = [c for c in cells for _ in range(v)] if i % 2 else [c for _ in range(v) for c in cells]
        f = still(n, rng, width, height)
        frames.append(junk_padding(plant(f, 20 + 7 * i, votes, block), rng))
    return frames


def test_row_wrap_and_edge_columns(gpu_scanner_factory, monkeypatch):
    """(119, y) and (0, y + 1) are adjacent in memory and no neighbours.  A pair that touches column 0 or 119 holds one
    centre (the inner cell), which is below CLUSTERS_NEEDED = 2: flag 0 by the reference, so the vote must not prove
    it; one column further in, the same pair holds two."""
    p = params_of()
    v = 2
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    y = 30
    cases = [([(119, y), (0, y + 1)], 0), ([(0, y + 1), (119, y)], 0),
             ([(0, y), (1, y)], 0), ([(1, y), (0, y)], 0), ([(118, y), (119, y)], 0), ([(119, y), (118, y)], 0),
             ([(1, y), (2, y)], 1), ([(117, y), (118, y)], 1), ([(2, y), (1, y)], 1),
             ([(0, y), (0, y + 1)], 0), ([(119, y), (119, y + 1)], 0), ([(1, y), (1, y + 1)], 1), ([(118, y + 1), (118, y)], 1),
             ([(0, y), (1, y), (119, y - 1)], 0), ([(0, y), (1, y), (2, y)], 1), ([(119, y), (118, y), (117, y)], 1),
             ([(50, 2), (50, 3)], 0), ([(50, 3), (50, 2)], 0), ([(50, 64), (50, 65)], 0), ([(50, 65), (50, 64)], 0),
             ([(50, 3), (50, 4)], 1), ([(50, 64), (50, 63)], 1), ([(50, 3), (51, 3)], 1), ([(50, 64), (51, 64)], 1),
             ([(50, 2), (51, 2)], 0), ([(50, 65), (51, 65)], 0)]
    rng = np.random.RandomState(77)
    mv, off, sd = batch_of(geometry_frames(v, [c for c, _ in cases], rng))
    want_f, _ = three_way(on, off_, p, mv, off, sd, "row wrap / edge columns")
    assert want_f.tolist() == [w for _, w in cases]


def test_one_centre_is_enough_for_clusters_needed_1(gpu_scanner_factory, monkeypatch):
    """CLUSTERS_NEEDED 0 and 1: one centre decides.  (0, y) + (1, y) is one centre — flag 1 here, through the cluster
    test, since the proof asks for two."""
    rng = np.random.RandomState(78)
    for cn in (0, 1):
        p = params_of(clusters_needed=cn)
        on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
        cases = [([(0, 30), (1, 30)], 1), ([(119, 30), (0, 31)], 0), ([(60, 30), (61, 30)], 1), ([(60, 30), (62, 30)], 0),
                 ([(0, 30), (0, 31)], 0)]
        mv, off, sd = batch_of(geometry_frames(2, [c for c, _ in cases], rng))
        want_f, _ = three_way(on, off_, p, mv, off, sd, f"clusters_needed {cn}")
        assert want_f.tolist() == [w for _, w in cases]


def test_without_a_vertical_mask(gpu_scanner_factory, monkeypatch):
    """vertical_mask 0: rows 0 and gh - 1 are analysed and have no row above / below them in the tile."""
    p = params_of(vertical_mask=0.0)
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    cases = [[(5, 0), (6, 0)], [(5, 0), (5, 1)], [(5, 1), (5, 0)], [(5, 67), (6, 67)], [(5, 66), (5, 67)], [(5, 67), (5, 66)],
             [(119, 0), (0, 1)], [(0, 0), (1, 0)], [(118, 67), (119, 67)], [(1, 0), (2, 0)], [(117, 67), (118, 67)],
             [(0, 0)], [(119, 67)], [(1, 0)], [(118, 67)], [(119, 66), (0, 67)]]
    rng = np.random.RandomState(79)
    mv, off, sd = batch_of(geometry_frames(2, cases, rng))
    want_f, _ = three_way(on, off_, p, mv, off, sd, "vertical_mask 0")
    assert want_f.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0]


def test_checkerboard_never_exits(gpu_scanner_factory, monkeypatch):
    """Every other cell of every other row is active, none has an active neighbour: flag 0 after a full read, also when
    one more vote lands on an active cell; one frame with a single extra cell that joins two of them is decided."""
    p = params_of()
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    rng = np.random.RandomState(80)
    board = [(x, y) for y in range(3, 65, 2) for x in range(0, GW, 2)]
    frames = []
    for extra in ([], [(50, 31)] * 3, [(51, 31)] * 2, [(50, 32)] * 2, [(51, 31)]):
        votes = [c for c in board for _ in range(2)] + extra
        order = rng.permutation(len(votes))
        f = still(len(votes) + 500, rng)
        frames.append(junk_padding(plant(f, 100, [votes[i] for i in order]), rng))
    mv, off, sd = batch_of(frames)
    want_f, want_c = three_way(on, off_, p, mv, off, sd, "checkerboard")
    assert want_f.tolist() == [0, 0, 1, 1, 0] and want_c[0] == 0


@pytest.mark.parametrize("cn", [2, 3])
def test_clusters_needed_3_leaves_the_exit_off(gpu_scanner_factory, monkeypatch, cn):
    p = params_of(clusters_needed=cn)
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, cn <= 2)
    rng = np.random.RandomState(81)
    cases = [([(50, 30), (51, 30)], 1 if cn <= 2 else 0), ([(50, 30), (51, 30), (52, 30)], 1), ([(50, 30), (52, 30)], 0),
             ([(50, 30), (51, 30), (70, 40), (70, 41)], 1)]
    mv, off, sd = batch_of(geometry_frames(2, [c for c, _ in cases], rng))
    want_f, _ = three_way(on, off_, p, mv, off, sd, f"clusters_needed {cn}")
    assert want_f.tolist() == [w for _, w in cases]


def test_other_plans_leave_the_exit_off(gpu_scanner_factory, monkeypatch):
    """vectors_needed 0 (every cell is active without a vote) and packed counters: the plan key says off."""
    for kw, force in ((dict(vectors_needed=0), None), (dict(), 108), (dict(vectors_needed=1), 1)):
        p = params_of(**kw)
        s = gpu_scanner_factory(p, force_fb=force)
        assert early_exit.plan(s)["early_exit"] == 0, (kw, force, early_exit.plan(s))
    # no knob set: key 1, and a launch of a few frames (fewer than eight per CU) reads them to the end — flags as the oracle's
    monkeypatch.delenv("MTGPU_EARLY_EXIT", raising=False)
    p = params_of()
    s = gpu_scanner_factory(p)
    assert early_exit.plan(s)["early_exit"] == 1
    mv, off, sd = batch_of(geometry_frames(2, [[(50, 30), (51, 30)], [(0, 30), (1, 30)], [(50, 30)]], np.random.RandomState(85)))
    assert s.check_frames(m.FrameBatch(mv, off, None, sd)).tolist() == ob.scan_frames(p, mv, off, sd).tolist() == [1, 0, 0]
    assert early_exit.preview(m.ScanParams.from_config(1920, 1080))["early_exit"] == 1
    assert early_exit.preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))["early_exit"] == 0


# ------------------------------------------------------------------ several frames per workgroup, slices, pinned flags

def test_grouped_small_frames(gpu_scanner_factory, monkeypatch):
    """480p frames (40 x 30 cells), four per workgroup: decided and still frames alternate; a still frame right after a
    decided one in the same workgroup is 0.  Pairs of frames of 2600 records (longer than a streaming step: they take
    the exit) alternate with pairs of 1200 (dense16, one record per cell: all loads are issued before the first vote,
    so they take the plain votes), so a workgroup goes from one kind to the other and back."""
    p = params_of(640, 480, vectors_needed=1)
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True, MTGPU_GROUP=4)
    rng = np.random.RandomState(82)
    frames = []
    for i in range(64):
        f = still(2600 if (i // 2) % 2 == 0 else 1200, rng, 640, 480)
        if i % 2 == 0 or i % 8 == 5:
            plant(f, (97 * i) % 1100, [(10 + i % 20, 5 + i % 20), (11 + i % 20, 5 + i % 20)])
        elif i % 8 == 3:
            plant(f, 50, [(10, 10), (12, 10)])
        frames.append(junk_padding(f, rng))
    mv, off, sd = batch_of(frames)
    want_f, _ = three_way(on, off_, p, mv, off, sd, "group 4")
    assert want_f.tolist() == [1 if (i % 2 == 0 or i % 8 == 5) else 0 for i in range(64)]


def test_sliced_launches_and_pinned_flags(gpu_scanner_factory, monkeypatch):
    """A few large frames cut into slices (the exit is off for that launch: a slice sees only its share of the votes),
    and the unsliced launch with its flags in pinned host memory."""
    p = params_of()
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    rng = np.random.RandomState(83)
    n = 32640
    frames = []
    for i in range(6):
        f = still(n, rng)
        if i % 3 == 0:                                  # the pair's votes lie in different slices
            plant(f, 100, [(50, 30)] * 2)
            plant(f, n - 100, [(51, 30)] * 2)
        elif i % 3 == 1:
            plant(f, n // 2 + 7, pair_votes((50, 30), (51, 30), 2))
        frames.append(junk_padding(f, rng))
    mv, off, sd = batch_of(frames)
    for slices in (0, 2, 8, 1):
        on.set_slices(slices)
        off_.set_slices(slices)
        want_f, _ = three_way(on, off_, p, mv, off, sd, f"slices {slices}", pinned=(slices == 1))
        assert want_f.tolist() == [1, 1, 0, 1, 1, 0]


def test_few_frames_on_the_wide_layout(gpu_scanner_factory, monkeypatch):
    """A 64 x 314 grid of 32-bit counters: launches of at most one frame per CU take the single-chunk mask buffer, which
    moves the words behind it (the `decided` word among them); larger launches take the chunked layout."""
    p = params_of(1024, 5024, vertical_mask=0.0)
    assert (p.grid_w, p.grid_h) == (64, 314)
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True)
    assert on.plan["counter_bits"] == 32 and on.plan["bands"] == 1 and on.plan["chunk_rows"] < 314, on.plan
    rng = np.random.RandomState(84)
    cases = [[(5, 0), (6, 0)], [(5, 313), (5, 312)], [(0, 100), (1, 100)], [(63, 100), (0, 101)], [(30, 200), (30, 201)],
             [(30, 200), (32, 200)], [(62, 313), (63, 313)], [(61, 313), (62, 313)]]
    want = [1, 1, 0, 0, 1, 0, 0, 1]
    few = geometry_frames(2, cases, rng, width=1024, height=5024)
    mv, off, sd = batch_of(few)
    want_f, _ = three_way(on, off_, p, mv, off, sd, "wide layout")
    assert want_f.tolist() == want
    reps = on.plan["cu_count"] // len(few) + 2
    mv, off, sd = batch_of(few * reps)
    want_f, _ = three_way(on, off_, p, mv, off, sd, "chunked layout")
    assert want_f.tolist() == want * reps


# ------------------------------------------------------------------ the bytes are really skipped

def test_decided_frames_are_not_read_to_the_end(gpu_scanner_factory, monkeypatch):
    """2048 frames of 1.3 MB (1080p, four records per cell in raster order), the deciding pair in the first analysed
    row: its votes are records 1480 .. 1487 of 32 640, inside the first of the frame's sixteen streaming steps, so a
    workgroup that polls once per step reads at most two of them.  Scan-kernel time from the library's profile events,
    mean of 10 launches after warm-up, exit on and exit off alternating in one process: on < 0.5 x off — a factor of four
    above the byte ratio, for the per-workgroup fixed cost and the dispatch rate.  A condition, not a benchmark."""
    import torch
    p = params_of()
    on, off_ = scanners(gpu_scanner_factory, monkeypatch, p, True, any_size=False)     # the default: no knob set
    cells = np.arange(GW * GH).repeat(4)
    f = np.zeros(len(cells), dtype=m.MV_DTYPE)
    f["dst_x"] = (cells % GW) * 16 + 4
    f["dst_y"] = (cells // GW) * 16 + 4
    f["src_x"], f["src_y"] = f["dst_x"], f["dst_y"]
    moving = (cells // GW == 3) & ((cells % GW == 10) | (cells % GW == 11))
    f["src_x"][moving] -= 7
    assert len(f) == 32640 and np.flatnonzero(moving).tolist() == list(range(1480, 1488))
    assert ob.scan_frames(p, f, np.array([0, len(f)], dtype=np.uint64)).tolist() == [1]
    n_frames = 2048
    assert n_frames >= 8 * on.plan["cu_count"]           # the default takes the exit; one workgroup per CU, as on the headline
    d_mv = torch.from_numpy(f.view(np.uint8).copy()).cuda().repeat(n_frames)
    d_off = torch.arange(n_frames + 1, dtype=torch.int64, device="cuda") * len(f)
    flags = torch.empty(n_frames, dtype=torch.uint8, device="cuda")
    ms = {}
    for rnd in range(3):                                 # round 0 is the warm-up
        for name, s in (("on", on), ("off", off_)):
            s.profile(True)
            for _ in range(5):
                s.check_frames_device(d_mv, d_off, None, flags)
            pr = s.profile_read()
            s.profile(False)
            torch.cuda.synchronize()
            assert bool((flags == 1).all()), name
            if rnd:
                ms.setdefault(name, []).append(pr["scan_ms"])
    t_on, t_off = float(np.mean(ms["on"])), float(np.mean(ms["off"]))
    print(f"scan kernel ms, 2048 decided frames: exit on {t_on:.4f}, off {t_off:.4f}, ratio {t_on / t_off:.3f}")
    assert t_on < 0.5 * t_off, (t_on, t_off)
