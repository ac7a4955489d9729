"""Shared by the GPU test modules: GPU-vs-oracle parity of the scan ON THE CENTRE COUNT.

The flag of a frame is one bit of its centre count n (n >= max(1, CLUSTERS_NEEDED)), at a threshold that is nearly
always 1 or 2 on inputs whose counts are mostly far above it; the library also hands n itself out.  So every scan
that a test compares with the oracle is compared count for count: one oracle pass (ob.scan_centres) gives the
expected flags and counts, the host entry point (count_centres) always runs, and batches below a cost limit also go
through the device entry point on 40-byte and on compact records with junk-filled outputs.
"""
import numpy as np

import mvtrim_amd as m

import oracle_binding as ob

# Cost limit of the two extra device-entry legs (an upload of the batch in each layout plus two scans): batches with
# more records or frames than this are checked through the host entry point only, unless the caller asks for the
# device legs itself.  It limits run time, not coverage: every test that is ABOUT the device entry points or about a
# large batch calls device_centres() / count_centres_device() on its own tensors.
DEVICE_LEG_MAX_RECORDS = 400_000
DEVICE_LEG_MAX_FRAMES = 4_096


def to_device(mv, off, has_sd, compact):
    import torch
    raw = (m.pack_records(mv) if compact else np.ascontiguousarray(mv, dtype=m.MV_DTYPE)).view(np.uint8).reshape(-1)
    d_rec = torch.from_numpy(raw.copy()).cuda() if raw.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()
    d_sd = None if has_sd is None else torch.from_numpy(np.ascontiguousarray(has_sd, dtype=np.uint8)).cuda()
    return d_rec, d_off, d_sd


def junk_outputs(n):
    """(flags, centres) device tensors pre-filled with junk: every element must be written by the call."""
    import torch
    return (torch.full((n,), 9, dtype=torch.uint8, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda"))


def device_centres(s, mv, off, has_sd, compact, want_flags=True):
    """Through mtgpu_scan_centres_device, outputs pre-filled with junk: every element must be written."""
    d_rec, d_off, d_sd = to_device(mv, off, has_sd, compact)
    return device_centres_of(s, d_rec, d_off, d_sd, compact, want_flags)


def device_centres_of(s, d_rec, d_off, d_sd, compact, want_flags=True, stream=None):
    """The same on tensors that are on the device already -> (flags uint8 [F] or None, centres uint32 [F]) on the host."""
    import torch
    n = d_off.numel() - 1
    flags, centres = junk_outputs(n)
    fl, ce = s.count_centres_device(d_rec, d_off, d_sd, compact=compact, flags=flags if want_flags else False,
                                    centres=centres, stream=stream)
    torch.cuda.synchronize()
    return (None if fl is None else fl.cpu().numpy()), ce.cpu().numpy().view(np.uint32)


def assert_counts_equal(got_c, want_c, what, plan=None, got_f=None, want_f=None):
    """Element for element; the first differing frames are printed with want / got / plan."""
    got_c, want_c = np.asarray(got_c).astype(np.int64), np.asarray(want_c).astype(np.int64)
    assert got_c.shape == want_c.shape, (what, got_c.shape, want_c.shape)
    bad = np.flatnonzero(got_c != want_c)
    assert bad.size == 0, (f"{what}: centre counts of {bad.size} of {want_c.size} frames differ, first {bad[:8].tolist()}: "
                           f"want {want_c[bad[:8]].tolist()} got {got_c[bad[:8]].tolist()} plan {plan}")
    if want_f is not None:
        got_f, want_f = np.asarray(got_f), np.asarray(want_f)
        badf = np.flatnonzero(got_f != want_f)
        assert badf.size == 0, (f"{what}: flags of {badf.size} frames differ, first {badf[:8].tolist()}: "
                                f"want {want_f[badf[:8]].tolist()} got {got_f[badf[:8]].tolist()} plan {plan}")


def assert_centres_parity(scanner, params, mv, off, has_sd, plain_flags=None, want=None, nthreads=1, device=None,
                          what=""):
    """The centre counts of scanner.count_centres() (mtgpu_scan_frames_centres) equal the oracle's, frame by frame; its
    flags equal the oracle's and, if given, `plain_flags` (what check_frames returned for the same batch).
    `want`: (flags, centres) of an oracle pass the caller has made already.  `device`: None = the two device legs run
    for batches within the cost limit above, True / False = the caller decides.  `off` may be a window of a larger
    batch (it need not start at 0).  Returns the oracle's (flags, centres)."""
    want_f, want_c = ob.scan_centres(params, mv, off, has_sd, nthreads=nthreads) if want is None else want
    plan = scanner.plan
    flags2, centres = scanner.count_centres(m.FrameBatch(mv, off, None, has_sd))
    assert centres.dtype == np.uint32
    assert_counts_equal(centres, want_c, what + " host entry", plan, flags2, want_f)
    if plain_flags is not None:
        assert np.array_equal(flags2, plain_flags), (what, "flags of the centres call differ from the plain call's", plan)
    n_frames = len(off) - 1
    if device is None:
        device = n_frames <= DEVICE_LEG_MAX_FRAMES and int(off[-1]) - int(off[0]) <= DEVICE_LEG_MAX_RECORDS and \
            len(mv) <= 4 * DEVICE_LEG_MAX_RECORDS
    if device and n_frames > 0:
        for compact in (False, True):
            fl, ce = device_centres(scanner, mv, off, has_sd, compact)
            assert_counts_equal(ce, want_c, what + (" device entry, compact" if compact else " device entry, 40-byte"),
                                plan, fl, want_f)
    return want_f, want_c


def junk_padding(mv, rng):
    """Fill the padding bytes of the records (14-15, 34-39) with junk: the scan must ignore them."""
    raw = mv.view(np.uint8).reshape(-1, 40)
    if len(raw):
        raw[:, 14:16] = rng.randint(0, 256, size=(len(raw), 2))
        raw[:, 34:40] = rng.randint(0, 256, size=(len(raw), 6))
    return mv


# ------------------------------------------------------------------ the inputs of test_scan_edge_configs

EDGE_CFGS = [
    # (width, height, kwargs)
    (1920, 1080, dict()),
    (1920, 1080, dict(vertical_mask=0.0)),                              # margin 0: grid edges are centres
    (1920, 1080, dict(vectors_needed=1, clusters_needed=1)),
    (1920, 1080, dict(vectors_needed=0)),                               # every cell active
    (1920, 1080, dict(vectors_needed=255)),
    (1920, 1080, dict(vectors_needed=256 + 3)),                         # uint8 wrap -> 3
    (1920, 1080, dict(clusters_needed=0)), (1920, 1080, dict(clusters_needed=-5)),
    (1920, 1080, dict(clusters_needed=100000)),
    (1920, 1080, dict(mv_threshold_sq=0.0)), (1920, 1080, dict(mv_threshold_sq=-1.0)),
    (1920, 1080, dict(mv_threshold_sq=float("nan"))), (1920, 1080, dict(mv_threshold_sq=float("inf"))),
    (1920, 1080, dict(mv_threshold_sq=24.5)), (1920, 1080, dict(mv_threshold_sq=25.0)),
    (1920, 1080, dict(mv_threshold_sq=2.0e9)),
    (1920, 1080, dict(vertical_mask=0.5)), (1920, 1080, dict(vertical_mask=0.6)),   # empty analysed range
    (16, 16, dict(vertical_mask=0.0)), (32, 48, dict(vertical_mask=0.0)), (48, 48, dict(vertical_mask=0.0)),
    (1008, 64, dict(vertical_mask=0.0)), (1024, 64, dict(vertical_mask=0.0)),       # gw 63, 64
    (1040, 64, dict(vertical_mask=0.0)), (2064, 96, dict()),                         # gw 65, 129
    (1920, 1080, dict(block_size=8, block_shift=3)),                                 # 240x135 on 1080p
    (1920, 1080, dict(block_size=16, block_shift=5)),                                # size/shift mismatch
    (640, 480, dict(block_size=1, block_shift=0, vectors_needed=1)),                 # 640x480 cells
    (32767, 3, dict(block_size=1, block_shift=0, vectors_needed=1, vertical_mask=0.0)),   # widest legal grid
    (3, 32767, dict(block_size=1, block_shift=0, vectors_needed=1, vertical_mask=0.0)),   # tallest: chunked masks
    (32767, 40, dict(block_size=1, block_shift=0, vectors_needed=2, clusters_needed=1)),  # wide + row bands
]

# The sets on which no frame can have a centre at all, with the reason; tests/test_scan_inputs.py lets no other set
# through without frames that count something, and fails if this list grows.
EDGE_CFGS_WITHOUT_CENTRES = [
    ((1920, 1080, dict(mv_threshold_sq=float("inf"))), "no record passes the threshold"),
    ((1920, 1080, dict(mv_threshold_sq=2.0e9)), "only |d|^2 >= 2.0e9 passes: both differences beyond 31 600, twice per cell"),
    ((1920, 1080, dict(vertical_mask=0.5)), "empty analysed range"),
    ((1920, 1080, dict(vertical_mask=0.6)), "empty analysed range"),
    ((16, 16, dict(vertical_mask=0.0)), "grid width 1: no column in [1, gw - 2]"),
    ((32, 48, dict(vertical_mask=0.0)), "grid width 2: no column in [1, gw - 2]"),
]


def cells_frame(cells, dx=5):
    """One record per vote: cells = [(x, y, votes)], (x, y) = a pixel inside the cell (the records' dst), |d|^2 = dx^2."""
    recs = [(x, y) for x, y, votes in cells for _ in range(votes)]
    mv = np.zeros(len(recs), dtype=m.MV_DTYPE)
    a = np.array(recs, dtype=np.int64).reshape(-1, 2)
    mv["dst_x"], mv["dst_y"] = a[:, 0], a[:, 1]
    mv["src_x"], mv["src_y"] = a[:, 0] - dx, a[:, 1]
    return mv


def _planted_vectors_needed_255():
    """1920 x 1080, 16-pixel cells (120 x 68, margin 3), VECTORS_NEEDED 255: a horizontal run of L adjacent cells in
    one row, 255 or more votes each -> every cell of the run is a centre: L.  Frame k: L = 2 + k % 5, row 5 + 4 k,
    from column 3 + 7 k; a 254-vote cell next to the run (one short) and a lone 300-vote cell two columns further
    change nothing."""
    frames, hand = [], []
    for k in range(12):
        run, row, col = 2 + k % 5, 5 + 4 * k, 3 + 7 * k
        cells = [((col + i) * 16 + 8, row * 16 + 8, 255 + (i * 37 + k) % 120) for i in range(run)]
        cells.append(((col + run) * 16 + 8, row * 16 + 8, 254))
        cells.append(((col + run + 2) * 16 + 8, row * 16 + 8, 300))
        frames.append(cells_frame(cells))
        hand.append(run)
    return frames, hand


def _planted_wide_row_bands():
    """32767 x 40 cells of one pixel (margin 2: centre rows 2 .. 37), VECTORS_NEEDED 2.  Frame j holds vertical pairs
    (x, r) + (x, r + 1), 2 or 3 votes per cell, for r = 2 + j % 3, 5 + j % 3, ... (the first j // 3 left out), each
    pair in a column of its own, 50 apart: 2 centres per pair.  Over the frames every row boundary 2|3 .. 36|37
    carries a pair, so wherever a plan puts its band seams, a pair sits on each of them, its two centres counted by
    different bands.  Odd frames add a horizontal pair across the 64-bit word boundary (63, 10) + (64, 10): 2 more,
    and one in the last two columns (32765, 20) + (32766, 20): 1 more, the last column never being a centre.  Frame 12
    is one column through all 36 centre rows: 36."""
    frames, hand = [], []
    for j in range(12):
        rows = list(range(2 + j % 3, 37, 3))[j // 3:]
        cells, n = [], 0
        for r in rows:
            x = 1000 + 50 * r + j
            cells += [(x, r, 2 + j % 2), (x, r + 1, 2 + (j + r) % 2)]
            n += 2
        if j % 2:
            cells += [(63, 10, 2), (64, 10, 2), (32765, 20, 3), (32766, 20, 2)]
            n += 3
        frames.append(cells_frame(cells))
        hand.append(n)
    frames.append(cells_frame([(20000, r, 2) for r in range(2, 38)]))
    hand.append(36)
    return frames, hand


PLANTED = [((1920, 1080, dict(vectors_needed=255)), _planted_vectors_needed_255),
           ((32767, 40, dict(block_size=1, block_shift=0, vectors_needed=2, clusters_needed=1)), _planted_wide_row_bands)]


def edge_config_inputs(width, height, kw):
    """(mv, off, has_sd, planted): the 48 random frames of this parameter set, seeded by the set itself, with junk in
    the records' padding bytes.  On the two sets whose random frames hold no centre at all, frames built by hand
    follow them (records shuffled inside each frame); `planted` = their centre counts, derived by hand (else [])."""
    import zlib
    from mvtrim_amd import synth
    seed = zlib.crc32(repr((width, height, sorted(kw.items()))).encode()) % (2 ** 31)
    rng = np.random.RandomState(seed)
    mv, off, sd = synth.random_frames(rng, 48, 3000, width, height)
    junk_padding(mv, rng)
    make = [fn for cfg, fn in PLANTED if cfg == (width, height, kw)]
    if not make:
        return mv, off, sd, []
    frames, hand = make[0]()
    rng2 = np.random.RandomState(seed ^ 0x5A5A)
    frames = [junk_padding(f[rng2.permutation(len(f))], rng2) for f in frames]
    counts = np.array([len(f) for f in frames], dtype=np.uint64)
    off = np.concatenate([off, off[-1] + np.cumsum(counts)]).astype(np.uint64)
    mv = np.concatenate([mv] + frames)
    sd = np.concatenate([sd, np.ones(len(frames), dtype=np.uint8)])
    return mv, off, sd, hand

def pair_centres(votes, vec):
    """Hand value for frames built from pairs of adjacent cells that are far from every other voting cell: `votes` is
    a list of (n_a, n_b), the votes of the two cells of a pair (both inside the analysed rows, neither in column 0 or
    grid_w - 1).  A pair contributes 2 centres when both cells hold >= vec votes (each is active with an active
    4-neighbour), else 0: a lone active cell has no active neighbour."""
    return sum(2 for a, b in votes if min(a, 255) >= vec and min(b, 255) >= vec)
