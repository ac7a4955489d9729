"""GPU tier (`-m gpu`): direction planes — the per-cell allow byte and the flow map (include/mtgpu_lanes.h,
csrc/lanes_kernels.hip).

Every comparison is exact against tests/lanes_model.py, which tests/test_lanes_host.py ties to the unchanged oracle
through the record filter of consequence C and to the numbers written out by hand in tests/lanes_inputs.py; consequences
A, B and E are held against mtgpu_scan_dir_device, mtgpu_scan_centres_device and mtgpu_scan_zones_device (existing code)
bit for bit.  Outputs are pre-filled with junk: every element must be written by the call."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, lanes, tune, zones

import dir_inputs as di
import dir_model as dm
import lanes_inputs as li
import lanes_model as lm
from derived_edge_inputs import voters
from scan_checks import assert_counts_equal, device_centres_of, to_device
from test_gpu_dir import assert_equals_model, device_dir, junk_outputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG = -7, 9
NAMES = ("flags", "centres", "rose")


# ------------------------------------------------------------------ device helpers

def odd_planes(planes):
    """The planes on the device at an ODD byte address (a plane has no alignment), as a contiguous uint8 tensor."""
    import torch
    flat = np.ascontiguousarray(planes, dtype=np.uint8).reshape(-1)
    room = torch.zeros(flat.size + 1, dtype=torch.uint8, device="cuda")
    room[1:] = torch.from_numpy(flat.copy()).cuda()
    t = room[1:]
    assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    return t


def device_lanes(s, d_rec, d_off, d_sd, compact, planes, soff=None, stream=None, odd=True):
    """Through mtgpu_scan_lanes_device into junk-filled outputs -> (flags uint8 [F], centres uint32 [F], rose uint32
    [F, 8]) on the host."""
    import torch
    n = d_off.numel() - 1
    out = junk_outputs(n)
    d_soff = None if soff is None else torch.from_numpy(np.asarray(soff).astype(np.int64)).cuda()
    d_planes = odd_planes(planes) if odd else torch.from_numpy(np.ascontiguousarray(planes, dtype=np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    s.scan_lanes_device(d_rec, d_off, d_sd, d_planes, d_stream_off=d_soff, compact=compact, out=out, stream=stream)
    torch.cuda.synchronize()
    return (out["flags"].cpu().numpy(), out["centres"].cpu().numpy().view(np.uint32),
            out["rose"].cpu().numpy().view(np.uint32).reshape(n, 8))


def device_flow(s, d_rec, d_off, d_sd, compact, soff, fill=JUNK):
    """Through mtgpu_flow_map_device into a junk-filled map -> uint32 [S, 8, gh, gw] on the host."""
    import torch
    ns = len(soff) - 1
    out = torch.full((ns, 8, s.params.grid_h, s.params.grid_w), fill, dtype=torch.int32, device="cuda")
    d_soff = torch.from_numpy(np.asarray(soff).astype(np.int64)).cuda()
    torch.cuda.synchronize()
    s.flow_map_device(d_rec, d_off, d_sd, d_soff, compact=compact, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def assert_flow_equal(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {want.size} flow words differ, first (stream, sector, y, x) {bad[:6].tolist()}: "
                           f"want {[int(want[tuple(b)]) for b in bad[:6]]} got {[int(got[tuple(b)]) for b in bad[:6]]}")


CASES = dict(li.HAND_CASES, seam65=lambda: li.seam_case(65), seam129=lambda: li.seam_case(129), pieces=li.pieces_case,
             stream=li.stream_case, uhd_unstaged=lambda: li.uhd_case(0.0), uhd_staged=lambda: li.uhd_case(0.05))


@functools.lru_cache(maxsize=None)
def model_of(name):
    """The model's (flags, centres, rose) of a named case under its own planes: computed once."""
    c = CASES[name]()
    return lm.model_batch(c["params"], c["mv"], c["off"], c["sd"], c["planes"], c["soff"])


def whole_batch(c):
    return c["soff"] if c["soff"] is not None else np.array([0, len(c["off"]) - 1], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def flow_of(name):
    c = CASES[name]()
    return lm.flow_map(c["params"], c["mv"], c["off"], c["sd"], whole_batch(c))


def both_layouts(s, c, what, planes=None, soff="case"):
    """The case through the device entry point with both record sizes; yields (label, (flags, centres, rose))."""
    planes = c["planes"] if planes is None else planes
    soff = c["soff"] if isinstance(soff, str) else soff
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        yield f"{what}, {'compact' if compact else '40-byte'}", device_lanes(s, d_rec, d_off, d_sd, compact, planes, soff)


def flow_both_layouts(s, c, what, soff=None):
    soff = whole_batch(c) if soff is None else soff
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        yield f"{what}, {'compact' if compact else '40-byte'}", device_flow(s, d_rec, d_off, d_sd, compact, soff)


# ------------------------------------------------------------------ 1. frames derived by hand

@pytest.mark.parametrize("name", sorted(li.HAND_CASES))
def test_hand_frames(gpu_scanner_factory, name):
    """On the 6 x 5 grid: two records of different sectors in one cell; two of one sector in neighbouring cells whose bytes
    differ; a still record under threshold 0 and byte 0; vectors_needed 0; a record in a margin row whose byte is 0."""
    c = CASES[name]()
    s = gpu_scanner_factory(c["params"])
    want = model_of(name)
    assert want[1].tolist() == c["hand_centres"].tolist() and want[2].tolist() == c["hand_rose"].tolist()
    for label, got in both_layouts(s, c, name):
        assert_equals_model(got, want, label)
    # one plane for every frame, stream by stream, and the host entry point in both forms
    for st in range(len(c["planes"])):
        a, b = int(c["soff"][st]), int(c["soff"][st + 1])
        for label, got in both_layouts(s, c, f"{name}, plane {st} alone", planes=c["planes"][st], soff=None):
            assert got[1][a:b].tolist() == c["hand_centres"][a:b].tolist() and got[2][a:b].tolist() == c["hand_rose"][a:b].tolist(), label
    batch = m.FrameBatch(c["mv"], c["off"], None, c["sd"])
    res = s.scan_lanes(batch, c["planes"], stream_off=c["soff"])
    assert_equals_model((res["flags"], res["centres"], res["rose"]), want, name + ", host entry")
    assert res["rose"].dtype == np.uint32 and res["rose"].shape == (len(c["sd"]), 8)
    res = s.scan_lanes(batch, c["planes"][0])
    assert res["centres"][0] == c["hand_centres"][0]
    # the flow map of the same records
    for label, got in flow_both_layouts(s, c, name + ", flow map"):
        assert_flow_equal(got, flow_of(name), label)
    assert_flow_equal(s.flow_map(batch, c["soff"]), flow_of(name), name + ", flow map, host entry")


# ------------------------------------------------------------------ 2. consequences A and B on the streamers' edges

def test_uniform_planes_on_the_streamer_edges(gpu_scanner_factory):
    """dir_inputs.edge_case — frames of 0, 1, 2, 15, 16, 17, 4095 .. 8207 records on all sixteen 8-byte phases — both record
    sizes.  A: a plane filled with one byte is mtgpu_scan_dir_device under that byte, bit for bit.  B: a plane of 0xFF is
    mtgpu_scan_centres_device.  G: the flow map's sums are the roses' sums."""
    c = di.edge_case()
    p = c["params"]
    s = gpu_scanner_factory(p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        assert d_rec.data_ptr() % 128 == 0                          # the phases of dir_inputs.edge_case rest on it
        for byte in (di.EDGE_ALLOW, 0xFF):
            want = device_dir(s, d_rec, d_off, d_sd, compact, allow=byte)
            got = device_lanes(s, d_rec, d_off, d_sd, compact, np.full((p.grid_h, p.grid_w), byte, dtype=np.uint8))
            assert_equals_model(got, want, f"uniform plane {byte:#x}, compact {compact}")
        assert got[2].tolist() == c["hand_rose"].tolist()
        plain_f, plain_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        assert_counts_equal(got[1], plain_c, f"plane 0xFF against the centre scan, compact {compact}", got_f=got[0], want_f=plain_f)
        flow = device_flow(s, d_rec, d_off, d_sd, compact, [0, len(c["sd"])])
        assert flow[0].sum(axis=(1, 2)).tolist() == got[2].sum(axis=0).tolist()
    # per-stream uniform planes give the values of per-stream bytes
    c = di.boundary_case()
    s = gpu_scanner_factory(c["params"])
    planes = np.stack([np.full((c["params"].grid_h, c["params"].grid_w), a, dtype=np.uint8) for a in c["allows"]])
    d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], True)
    want = device_dir(s, d_rec, d_off, d_sd, True, soff=c["soff"], allows=c["allows"])
    assert_equals_model(device_lanes(s, d_rec, d_off, d_sd, True, planes, c["soff"]), want, "per-stream uniform planes")
    assert want[1].tolist() == di.BOUNDARY_HAND


def test_unaligned_40_byte_base(gpu_scanner_factory):
    """(base & 7) != 0 takes stream_mv40's branch without a head peel, here with lanes_vote and flow_count at 1024 lanes
    and four loads in flight: the batch of test_uniform_planes_on_the_streamer_edges as 40-byte records at byte shifts 4,
    12 and 20.  The plane scan under a plane whose bytes differ cell by cell, one plane for every frame and one per
    stream (five frames lie behind the last stream), and the flow map over the same streams, against the models.  An odd
    base is MT_ERR_INVALID and writes nothing: asserted here for both entry points — tests/api_arg_rungs.py holds neither
    mtgpu_scan_lanes_device nor mtgpu_flow_map_device."""
    import torch
    from test_gpu_derived_edges import shifted
    from derived_edge_inputs import UNALIGNED_SHIFTS
    c = di.edge_case()
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    F = len(sd)
    s = gpu_scanner_factory(p)
    soff = np.array([0, F // 3, F // 2, F - 5], dtype=np.uint64)
    one = li.cellwise_plane(p)
    planes = np.stack([one, np.full_like(one, di.EDGE_ALLOW), one ^ 0xFF])
    want_one, want_streams = lm.model_batch(p, mv, off, sd, one), lm.model_batch(p, mv, off, sd, planes, soff)
    want_flow = lm.flow_map(p, mv, off, sd, soff)
    assert want_one[2].tolist() == c["hand_rose"].tolist() and (want_one[1] > 0).any() and not want_streams[2][F - 5:].any()
    assert want_flow.sum(axis=(0, 2, 3)).tolist() == want_one[2][:F - 5].sum(axis=0, dtype=np.uint64).tolist()      # G
    raw = torch.from_numpy(mv.view(np.uint8).reshape(-1).copy())
    _, d_off, d_sd = to_device(mv[:0], off, sd, False)
    for shift in UNALIGNED_SHIFTS:
        d_rec = shifted(raw, shift)
        assert_equals_model(device_lanes(s, d_rec, d_off, d_sd, False, one), want_one, f"base shifted by {shift} bytes, one plane")
        assert_equals_model(device_lanes(s, d_rec, d_off, d_sd, False, planes, soff), want_streams, f"base shifted by {shift} bytes, per stream")
        assert_flow_equal(device_flow(s, d_rec, d_off, d_sd, False, soff), want_flow, f"base shifted by {shift} bytes, flow map")
    out = junk_outputs(F)
    flow = torch.full((3, 8, p.grid_h, p.grid_w), JUNK, dtype=torch.int32, device="cuda")
    odd = torch.zeros(raw.numel() + 8, dtype=torch.uint8, device="cuda")[1:1 + raw.numel()]
    d_planes, d_soff = odd_planes(planes), torch.from_numpy(soff.astype(np.int64)).cuda()
    lib = s._lib
    rc = lib.mtgpu_scan_lanes_device(s._ctx, odd.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), F, d_soff.data_ptr(), 3,
                                     d_planes.data_ptr(), out["flags"].data_ptr(), out["centres"].data_ptr(), out["rose"].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in lib.mtgpu_last_error().decode()
    rc = lib.mtgpu_flow_map_device(s._ctx, odd.data_ptr(), 40, len(mv), d_off.data_ptr(), d_sd.data_ptr(), F, d_soff.data_ptr(), 3,
                                   flow.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _abi.MT_ERR_INVALID and "4-byte" in lib.mtgpu_last_error().decode()
    assert all(int((t != (JUNK_FLAG if n == "flags" else JUNK)).sum()) == 0 for n, t in out.items()) and int((flow != JUNK).sum()) == 0


# ------------------------------------------------------------------ 3. word seams

@pytest.mark.parametrize("gw", [65, 129])
def test_word_seams(gpu_scanner_factory, gw):
    """Bytes change across columns 63 | 64 (and 127 | 128); two streams of 9 gw bytes, an odd number: plane 1 starts on an
    odd byte address whatever plane 0 starts on (both parities are run)."""
    name = f"seam{gw}"
    c = CASES[name]()
    s = gpu_scanner_factory(c["params"])
    want = model_of(name)
    assert want[1].tolist() == li.SEAM_HAND[gw]
    for label, got in both_layouts(s, c, name):
        assert_equals_model(got, want, label)
    d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], True)
    assert_equals_model(device_lanes(s, d_rec, d_off, d_sd, True, c["planes"], c["soff"], odd=False), want, name + ", plane 0 aligned")
    for label, got in flow_both_layouts(s, c, name + ", flow map"):
        assert_flow_equal(got, flow_of(name), label)


# ------------------------------------------------------------------ 4. the two forms on the 4K grid

@pytest.mark.parametrize("name", ["uhd_unstaged", "uhd_staged"])
def test_both_forms_on_the_4k_grid(gpu_scanner_factory, name):
    """240 x 135 cells and a plane whose bytes differ cell by cell.  Vertical mask 0: the plane is read from memory behind
    the vote's branch; 0.05: the same plane and records with its 123 analysed rows staged in LDS."""
    c = CASES[name]()
    assert m.lanes_preview(c["params"])["staged"] == (1 if name == "uhd_staged" else 0)
    s = gpu_scanner_factory(c["params"])
    want = model_of(name)
    assert (want[1] > 0).all()
    for label, got in both_layouts(s, c, name):
        assert_equals_model(got, want, label)
    for label, got in flow_both_layouts(s, c, name + ", flow map"):
        assert_flow_equal(got, flow_of(name), label)


# ------------------------------------------------------------------ 5. a frame in three pieces

def test_three_piece_frame(gpu_scanner_factory):
    """Frames of 300 000 records, three pieces of the kernel's 131 072, in one cell column; half of its cells forbid the
    records' sector."""
    c = CASES["pieces"]()
    s = gpu_scanner_factory(c["params"])
    want = model_of("pieces")
    assert want[1].tolist() == [3, 6] and want[2].tolist() == c["hand_rose"].tolist()
    for label, got in both_layouts(s, c, "three pieces"):
        assert_equals_model(got, want, label)
    for label, got in flow_both_layouts(s, c, "three pieces, flow map"):
        assert_flow_equal(got, flow_of("pieces"), label)
        assert got[:, li.PIECES_SECTOR, :, li.PIECES_COLUMN].tolist() == [[50000] * 6] * 2


# ------------------------------------------------------------------ 6. streams

def test_streams(gpu_scanner_factory):
    """Streams of 0, 1, 2, 64, 0, 0 and 33 frames with seven different planes; three frames in front of the first stream
    and five behind the last hold records and read 0 in outputs that start out non-zero; a key frame inside a stream; the
    one-plane form on the same batch; the host entry points on the frames up to the last stream's end."""
    c = CASES["stream"]()
    p = c["params"]
    s = gpu_scanner_factory(p)
    want = model_of("stream")
    F = len(c["sd"])
    orphan = np.r_[0:di.STREAM_FRONT, F - di.STREAM_BEHIND:F]
    for label, got in both_layouts(s, c, "streams"):
        assert_equals_model(got, want, label)
        assert not got[0][orphan].any() and not got[1][orphan].any() and not got[2][orphan].any(), label
        k = di.STREAM_KEY_FRAME
        assert got[0][k] == 0 and got[1][k] == 0 and not got[2][k].any(), label
    one = lm.model_batch(p, c["mv"], c["off"], c["sd"], c["planes"][6])
    for label, got in both_layouts(s, c, "one plane for every frame", planes=c["planes"][6], soff=None):
        assert_equals_model(got, one, label)
    assert (one[1][orphan] > 0).any()                              # the same frames count under the one-plane form
    for label, got in flow_both_layouts(s, c, "streams, flow map"):
        assert_flow_equal(got, flow_of("stream"), label)
        assert not got[0].any() and not got[4].any() and not got[5].any()
        # G against the rose of the same batch
        for st in range(len(c["planes"])):
            a, b = int(c["soff"][st]), int(c["soff"][st + 1])
            assert got[st].sum(axis=(1, 2)).tolist() == want[2][a:b].sum(axis=0, dtype=np.uint64).tolist(), (label, st)
    n = F - di.STREAM_BEHIND
    batch = m.FrameBatch(c["mv"][:int(c["off"][n])], c["off"][:n + 1], None, c["sd"][:n])
    res = s.scan_lanes(batch, c["planes"], stream_off=c["soff"])
    assert_equals_model((res["flags"], res["centres"], res["rose"]), tuple(w[:n] for w in want), "streams, host entry")
    assert_flow_equal(s.flow_map(batch, c["soff"]), flow_of("stream"), "streams, flow map, host entry")
    with pytest.raises(m.MtgpuError) as ei:                        # the host entry points want stream_off to end on n_frames
        s.scan_lanes(m.FrameBatch(c["mv"], c["off"], None, c["sd"]), c["planes"], stream_off=c["soff"])
    assert ei.value.code == _abi.MT_ERR_INVALID and "n_frames" in str(ei.value)


# ------------------------------------------------------------------ 7. the consequences on random draws

@pytest.mark.parametrize("i", range(li.N_DRAWS))
def test_consequences_on_random_draws(i):
    """Draw i (grids of the soak's set, vectors_needed i % 4, margin 0 .. 3, up to 12 frames of up to 3 000 records) with
    random planes, compact records on odd draws.  Every output equals the model's (which the CPU tier ties to the oracle
    through C).  D: a chain of growing planes.  E: a plane of 0x00 / 0xFF bytes against mtgpu_scan_zones_device.  F where
    vectors_needed is 0.  B at the chain's end.  The flow map of the first twenty draws equals the model's, and G."""
    import torch
    c = li.draw(i)
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    compact = bool(i % 2)
    F = len(sd)
    with m.MotionScanner(p, device=0) as s:
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        plain_f, plain_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        prev = None
        for j, plane in enumerate(c["chain"]):
            got = device_lanes(s, d_rec, d_off, d_sd, compact, plane)
            assert_equals_model(got, lm.model_batch(p, mv, off, sd, plane), f"draw {i} plane {j} of the chain")
            if prev is not None:
                assert (prev <= got[1]).all(), f"draw {i}: not monotone at plane {j}"                      # D
            prev = got[1]
            if p.vectors_needed == 0:
                assert_counts_equal(got[1], plain_c, f"draw {i} vn 0 plane {j}", got_f=got[0], want_f=plain_f)    # F
        assert_counts_equal(prev, plain_c, f"draw {i}: plane 0xFF against the centre scan", got_f=got[0], want_f=plain_f)   # B
        if p.vectors_needed >= 1 and p.mv_threshold_sq >= 1.0:                                             # E
            got = device_lanes(s, d_rec, d_off, d_sd, compact, c["zones"])
            d_soff = torch.tensor([0, F], dtype=torch.int64, device="cuda")
            d_keep = torch.from_numpy(zones.pack_keep(lm.zones_keep(c["zones"])).view(np.int64).copy()).reshape(1, p.grid_h, -1).cuda()
            zf, zc, _ = s.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, compact=compact)
            torch.cuda.synchronize()
            assert_counts_equal(got[1], zc.cpu().numpy().view(np.uint32), f"draw {i}: 0x00 / 0xFF plane against the masked scan",
                                got_f=got[0], want_f=zf.cpu().numpy())
        if i < li.N_FLOW_DRAWS:
            cut = F // 2
            for soff in ([0, F], [0, cut, F]):
                flow = device_flow(s, d_rec, d_off, d_sd, compact, soff)
                assert_flow_equal(flow, lm.flow_map(p, mv, off, sd, np.asarray(soff, dtype=np.uint64)), f"draw {i} flow map, streams {soff}")
            rose = device_lanes(s, d_rec, d_off, d_sd, compact, c["planes"])[2]
            assert flow[0].sum(axis=(1, 2)).tolist() == rose[:cut].sum(axis=0, dtype=np.uint64).tolist()   # G
            assert flow[1].sum(axis=(1, 2)).tolist() == rose[cut:].sum(axis=0, dtype=np.uint64).tolist()


# ------------------------------------------------------------------ 8. the flow map across batches, on dirty outputs

def test_flow_maps_add_across_batches_and_clear_first(gpu_scanner_factory):
    """Two halves of a batch add up to the whole; a map that starts out non-zero is cleared, whatever it held; frames
    outside every stream count nowhere; no frames and no records: a map of zeros."""
    import torch
    c = CASES["stream"]()
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    s = gpu_scanner_factory(p)
    F = len(sd)
    whole = lm.flow_map(p, mv, off, sd, np.array([0, F], dtype=np.uint64))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for fill in (JUNK, 0x7fffffff, 0):
            assert_flow_equal(device_flow(s, d_rec, d_off, d_sd, compact, [0, F], fill=fill), whole, f"whole batch over {fill:#x}")
        cut = 41
        first = device_flow(s, d_rec, d_off, d_sd, compact, [0, cut])          # frames behind the stream count nowhere
        second = device_flow(s, d_rec, d_off, d_sd, compact, [cut, F])         # ... and frames in front of it
        assert first.any() and second.any()
        assert_flow_equal(first + second, whole, f"two halves, compact {compact}")
        # the halves as batches of their own
        a_rec, a_off, a_sd = to_device(mv[:int(off[cut])], off[:cut + 1], sd[:cut], compact)
        b_rec, b_off, b_sd = to_device(mv[int(off[cut]):], off[cut:] - off[cut], sd[cut:], compact)
        parts = device_flow(s, a_rec, a_off, a_sd, compact, [0, cut]) + device_flow(s, b_rec, b_off, b_sd, compact, [0, F - cut])
        assert_flow_equal(parts, whole, f"two batches, compact {compact}")
    empty = device_flow(s, torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), None, True,
                        [0, 0, 0])
    assert empty.shape == (2, 8, p.grid_h, p.grid_w) and not empty.any()


# ------------------------------------------------------------------ 9. refusals and exact writes

def test_refusals_touch_nothing_and_the_next_call_succeeds(gpu_scanner_factory):
    """Every MT_ERR_INVALID / MT_ERR_UNSUPPORTED of the two device entry points with a live context: the argument is named,
    canaries on both sides of every output and the outputs themselves are untouched, and the call that follows succeeds.
    Then every combination of NULL outputs, n_frames == 0 and a non-default stream."""
    import torch
    c = CASES["stream"]()
    p, mv, off, sd, soff = c["params"], c["mv"], c["off"], c["sd"], c["soff"]
    want = dict(zip(NAMES, model_of("stream")))
    s = gpu_scanner_factory(p)
    lib = s._lib
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_soff = torch.from_numpy(soff.astype(np.int64)).cuda()
    d_planes = odd_planes(c["planes"])
    F, PAD, NS = len(off) - 1, 64, len(soff) - 1

    def run(names=NAMES, n_frames=F, rb=8, stream=None, ctx=None, over=None, so=True, ns=None, pl=True, off_ptr=None):
        b = junk_outputs(F, PAD)
        torch.cuda.synchronize()
        ptr = {n: (b[n][PAD:].data_ptr() if n in names else None) for n in NAMES}
        ptr.update(over or {})
        rc = lib.mtgpu_scan_lanes_device((ctx or s)._ctx, d_rec.data_ptr(), rb, len(mv), d_off.data_ptr() if off_ptr is None else off_ptr,
                                         d_sd.data_ptr(), n_frames, d_soff.data_ptr() if so else None, (NS if so else 0) if ns is None else ns,
                                         d_planes.data_ptr() if pl else None, ptr["flags"], ptr["centres"], ptr["rose"], stream)
        torch.cuda.synchronize()
        return rc, {n: t.cpu().numpy() for n, t in b.items()}, lib.mtgpu_last_error().decode()

    def untouched(raw, names=NAMES):
        return all((raw[n] == (JUNK_FLAG if n == "flags" else JUNK)).all() for n in names)

    def good(raw, names=NAMES):
        for n in NAMES:
            junk = JUNK_FLAG if n == "flags" else JUNK
            assert (raw[n][:PAD] == junk).all() and (raw[n][PAD + F:] == junk).all(), (names, n)
            if n in names:
                got = raw[n][PAD:PAD + F]
                assert np.array_equal(got if n == "flags" else got.view(np.uint32), want[n]), (names, n)
            else:
                assert untouched(raw, (n,)), (names, n)

    def refused(code, word, **kw):
        rc, raw, msg = run(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert untouched(raw), kw
        rc, raw, msg = run()                                        # the next call succeeds
        assert rc == _abi.MT_OK, msg
        good(raw)

    inv = _abi.MT_ERR_INVALID
    refused(inv, "d_planes is NULL", pl=False)
    refused(inv, "d_planes is NULL", pl=False, so=False)
    for rb in (0, 16, 41):
        refused(inv, "rec_bytes", rb=rb)
    refused(inv, "all NULL", names=())
    refused(inv, "d_frame_off is NULL", off_ptr=0)
    refused(inv, "d_frame_off must be 8-byte aligned", off_ptr=d_off.data_ptr() + 4)
    refused(inv, "d_stream_off is NULL", so=False, ns=7)
    refused(inv, "n_streams is 0", ns=0)
    pinned = torch.full((F * 8,), JUNK, dtype=torch.int32).pin_memory()
    for name in NAMES:
        refused(inv, "d_" + name + " is not memory of device", over={name: pinned.data_ptr()})
        assert int((pinned != JUNK).sum()) == 0
    refused(inv, "d_centres must be 4-byte aligned", over={"centres": junk_outputs(F)["centres"].data_ptr() + 2})
    refused(inv, "d_rose must be 4-byte aligned", over={"rose": junk_outputs(F)["rose"].data_ptr() + 1})
    big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    refused(_abi.MT_ERR_UNSUPPORTED, "960x540", ctx=big)
    with pytest.raises(m.MtgpuError) as ei:
        big.scan_lanes(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)), np.zeros((540, 960), dtype=np.uint8))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # every combination of NULL outputs
    for names in [NAMES, ("flags", "centres"), ("flags", "rose"), ("centres", "rose"), ("flags",), ("centres",), ("rose",)]:
        rc, raw, msg = run(names)
        assert rc == _abi.MT_OK, (names, msg)
        good(raw, names)
    # n_frames == 0: MT_OK, nothing written
    rc, raw, msg = run(n_frames=0)
    assert rc == _abi.MT_OK and untouched(raw)
    # a non-default stream
    st = torch.cuda.Stream()
    rc, raw, msg = run(stream=st.cuda_stream)
    assert rc == _abi.MT_OK, msg
    good(raw)

    # ---- the flow map
    words = NS * 8 * p.grid_h * p.grid_w
    wflow = flow_of("stream").reshape(-1)

    def frun(rb=8, ctx=None, flow_ptr=None, so=True, ns=NS, off_ptr=None, n_frames=F):
        b = torch.full((words + 2 * PAD,), JUNK, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = lib.mtgpu_flow_map_device((ctx or s)._ctx, d_rec.data_ptr(), rb, len(mv), d_off.data_ptr() if off_ptr is None else off_ptr,
                                       d_sd.data_ptr(), n_frames, d_soff.data_ptr() if so else None, ns,
                                       b[PAD:].data_ptr() if flow_ptr is None else flow_ptr, None)
        torch.cuda.synchronize()
        return rc, b.cpu().numpy(), lib.mtgpu_last_error().decode()

    def fgood(raw):
        assert (raw[:PAD] == JUNK).all() and (raw[PAD + words:] == JUNK).all()
        assert np.array_equal(raw[PAD:PAD + words].view(np.uint32), wflow)

    def frefused(code, word, **kw):
        rc, raw, msg = frun(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
        assert (raw == JUNK).all(), kw
        rc, raw, msg = frun()
        assert rc == _abi.MT_OK, msg
        fgood(raw)

    frefused(inv, "d_flow is NULL", flow_ptr=0)
    frefused(inv, "rec_bytes", rb=12)
    frefused(inv, "d_stream_off is NULL", so=False)
    frefused(inv, "d_frame_off is NULL", off_ptr=0)
    frefused(inv, "d_frame_off must be 8-byte aligned", off_ptr=d_off.data_ptr() + 4)
    frefused(inv, "d_flow must be 4-byte aligned", flow_ptr=torch.zeros(words + 1, dtype=torch.int32, device="cuda").data_ptr() + 2)
    host_map = torch.full((words,), JUNK, dtype=torch.int32).pin_memory()
    frefused(inv, "d_flow is not memory of device", flow_ptr=host_map.data_ptr())     # a pinned-host output: global atomics
    assert int((host_map != JUNK).sum()) == 0
    frefused(_abi.MT_ERR_UNSUPPORTED, "960x540", ctx=big)
    rc, raw, msg = frun(ns=0)                                       # no stream owns an output element
    assert rc == _abi.MT_OK and (raw == JUNK).all()


def test_contract_program_in_c(tmp_path):
    """tests/c/abi_lanes_canaries.c: the caller-sized buffers exactly as the header sizes them, from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_lanes_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_lanes_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all lanes buffers respected" in out.stdout


def test_plain_c_lanes_example(tmp_path):
    """examples/lanes_example.c: a car against its lane and one with it, from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "lanes_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lanes_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0xFF everywhere              20 frames kept, 2 segment(s)" in out.stdout
    assert "upper half: not E, NE, SE    10 frames kept, 1 segment(s)" in out.stdout


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    c = CASES["stream"]()
    s = gpu_scanner_factory(c["params"])
    d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_lanes(s, d_rec, d_off, d_sd, False, c["planes"], c["soff"])
        r = s.profile_read()
        flow = device_flow(s, d_rec, d_off, d_sd, False, c["soff"])
        r2 = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert r2["launches"] == 1 and r2["scan_ms"] > 0.0
    assert_equals_model(got, model_of("stream"), "profiled call")
    assert_flow_equal(flow, flow_of("stream"), "profiled flow map")


# ------------------------------------------------------------------ 10. the command: learn a plane, find the wrong way

def two_way_recording():
    """90 frames of a 320 x 160 picture (20 x 10 cells) at 25 fps.  An object is three cells in a row with two records each.
    Frames 0 .. 29, the learning stretch: one moves WEST along row 2 of the upper half and one EAST along row 7 of the
    lower half, each passing columns 2 .. 18.  Frames 40 .. 49: one moves EAST along row 2, against its half; frames
    60 .. 69: one moves WEST along row 7, against its half; frames 80 .. 89: both halves flow their usual way again."""
    def obj(col0, row, dx):
        return voters([(col0 + c, row, 2, dx, 0) for c in range(3)])
    frames = []
    for f in range(90):
        parts = []
        if f < 30:
            parts = [obj(2 + f // 2, 2, -6), obj(2 + f // 2, 7, 6)]
        elif 40 <= f < 50:
            parts = [obj(5 + (f - 40) // 2, 2, 6)]
        elif 60 <= f < 70:
            parts = [obj(5 + (f - 60) // 2, 7, -6)]
        elif f >= 80:
            parts = [obj(5 + (f - 80) // 2, 2, -6), obj(5 + (f - 80) // 2, 7, 6)]
        frames.append(np.concatenate(parts) if parts else np.zeros(0, dtype=m.MV_DTYPE))
    return frames


def test_end_to_end_command(gpu_scanner_factory, tmp_path):
    """A .mtmv written with mvfile; `python -m mvtrim_amd.lanes --learn --save-plane` in a fresh child process, then
    `--plane P --invert --elsewhere none --json`: the inverted plane keeps exactly the frames of an object that moves
    against its half.  The model decides the expected plane and frame sets; the hand values are stated next to them."""
    frames = two_way_recording()
    F = len(frames)
    path, plane_path = str(tmp_path / "road.mtmv"), str(tmp_path / "road.mtdir")
    m.mvfile.write_mtmv(path, 320, 160, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    cfg = dict(mv_threshold_sq=4.0, vectors_needed=2, clusters_needed=1, vertical_mask=0.0)
    p = m.ScanParams.from_config(320, 160, **cfg)
    assert (p.grid_w, p.grid_h, p.vertical_margin) == (20, 10, 0)
    batch, pts, hdr = tune.load(path)
    mv, off, sd = np.ascontiguousarray(batch.mv, dtype=m.MV_DTYPE), np.ascontiguousarray(batch.frame_off, dtype=np.uint64), batch.has_sd
    flow = lm.flow_map(p, mv, off, sd, np.array([0, F], dtype=np.uint64))[0]
    plane = lanes.plane_from_flow(flow, 4, 102, 1, 0xFF)
    # by hand: rows 2 and 7, columns 2 .. 18 are learned; west (with NW, SW) is usual in row 2, east (with NE, SE) in row 7
    hand = np.full((10, 20), 0xFF, dtype=np.uint8)
    hand[2, 2:19], hand[7, 2:19] = 0x38, 0x83
    assert np.array_equal(plane, hand)
    wrong = lanes.invert_plane(plane, plane != 0xFF, 0)
    want_all = lm.model_batch(p, mv, off, sd, np.full_like(plane, 0xFF))[0]
    want_wrong = lm.model_batch(p, mv, off, sd, wrong)[0]
    against = list(range(40, 50)) + list(range(60, 70))
    assert np.flatnonzero(want_wrong).tolist() == against and int(want_all.sum()) == 60
    s = gpu_scanner_factory(p)
    assert np.array_equal(s.flow_map(batch, [0, F])[0], flow)
    assert np.flatnonzero(s.scan_lanes(batch, wrong)["flags"]).tolist() == against

    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONIOENCODING="utf-8")
    common = ["--mv-threshold-sq", "4", "--vectors-needed", "2", "--clusters-needed", "1", "--vertical-mask", "0"]
    base = [sys.executable, "-m", "mvtrim_amd.lanes", path] + common
    out = subprocess.run(base + ["--learn", "--min-records", "4", "--share", "0.4", "--widen", "1", "--save-plane", plane_path],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    rows = [ln for ln in out.stdout.splitlines() if not ln.startswith("#")]
    assert len(rows) == 10 and all(len(r) == 20 for r in rows)
    assert rows[2] == "··" + "←" * 17 + "·" and rows[7] == "··" + "→" * 17 + "·" and rows[0] == "·" * 20
    assert np.array_equal(lanes.load_plane(plane_path, grid=(20, 10)), hand)
    out = subprocess.run(base + ["--plane", plane_path, "--invert", "--elsewhere", "none", "--json", "--max-gap-sec", "0.2",
                                 "--padding-sec", "0.04", "--min-savings-pct", "5"], capture_output=True, text=True, env=env, cwd=ROOT,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert doc["plane"]["frames"] == against and doc["plane"]["motion_frames"] == 20 and doc["plane"]["segments"] == 2
    assert doc["all"]["motion_frames"] == 60 and doc["all"]["segments"] == 4 and doc["restricted_cells"] == 34
    assert 0.0 < doc["plane"]["seconds_kept"] < doc["all"]["seconds_kept"] < F / 25.0
    # the same planes by hand, and the table, in this process
    assert lanes.main([path] + common + ["--lane", "2,2,19,3:E,NE,SE,S,N", "--lane", "2,7,19,8:W,NW,SW,S,N", "--unit", "cell",
                                         "--elsewhere", "none"]) == 0
