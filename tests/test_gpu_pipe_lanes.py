"""GPU tier (`-m gpu`): direction planes carried through the pipe under its keep mask (include/mtgpu_pipe_lanes.h;
csrc/lanes_kernels.hip, lanes_pipe_kernel), the C++ host layer and mtgpu_scan_file.  Expected values: numbers derived by
hand and the model (tests/pipe_lanes_inputs.py; both checked without a GPU by tests/test_pipe_lanes_host.py), and
mtgpu_scan_frames_lanes / the direction pipe / the plain and the masked pipe on the same frames for P1 - P6.  Every
comparison is exact."""
import contextlib
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, lanes, zones

import dir_inputs as di
import lanes_inputs as li
import pipe_dir_inputs as pd
import pipe_gmc_inputs as pg
import pipe_lanes_inputs as pl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES
# test_gpu_pipe_dir.py's LAYOUTS — compact8 / aos40 x copied / zero-copy — each with and without the centre counts
LAYOUTS = [rec | zc | ce for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC) for ce in (CE, 0)]
LAYOUT_IDS = ["-".join([r] + z + c) for r in ("compact8", "aos40") for z in ([], ["zero-copy"]) for c in (["centres"], [])]
SEC = _abi.MT_PIPE_REPORT_SECTORS


def feed_all(pipe, frames, pts=None):
    for i, f in enumerate(frames):
        pipe.feed(f, float(i) if pts is None else pts[i], tag=i)


def run(pipe, frames, pts=None):
    """Feed, drain -> (flags, counts) lists in tag order (the pipe returns submission order: asserted equal); counts is
    None in a pipe without MT_LAYOUT_CENTRES."""
    feed_all(pipe, frames, pts)
    if pipe._centres:
        out = pipe.drain_centres()
        assert [t for _, _, t, _ in out] == list(range(len(frames)))
        return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]
    out = pipe.drain()
    assert [t for _, _, t in out] == list(range(len(frames)))
    return [fl for _, fl, _ in out], None


def both(pipe, frames, plane):
    """(flags, centres, words) of a pipe with MT_LAYOUT_CENTRES under `plane`: one run per report; the flags agree."""
    pipe.set_plane(plane, "centres")
    got, rep = pipe.plane
    assert np.array_equal(got, plane) and rep == "centres"
    fl, ce = run(pipe, frames)
    pipe.set_plane(plane, "sectors")
    assert pipe.plane[1] == "sectors"
    fl2, wd = run(pipe, frames)
    assert fl == fl2
    return fl, ce, wd


def both_dir(pipe, frames, allow):
    """The same of the direction pipe under the byte `allow`; the pipe is left without a mode."""
    pipe.clear_plane()
    pipe.set_dir(allow, "centres")
    fl, ce = run(pipe, frames)
    pipe.set_dir(allow, "sectors")
    fl2, wd = run(pipe, frames)
    pipe.clear_dir()
    assert fl == fl2
    return fl, ce, wd


def resident(s, frames, plane):
    """mtgpu_scan_frames_lanes in its one-plane form on the same frames -> (flags, centres, words derived from its rose)."""
    r = s.scan_lanes(m.FrameBatch.from_frames(list(frames)), plane)
    return r["flags"].tolist(), r["centres"].tolist(), [direction.sector_word(x) for x in r["rose"].tolist()]


def resident_words(s, frames):
    r = s.scan_dir(m.FrameBatch.from_frames(list(frames)), 0xFF)
    return [direction.sector_word(x) for x in r["rose"].tolist()]


# ------------------------------------------------------------------ 1. the hand cases through the pipe

@pytest.mark.parametrize("name", list(li.HAND_CASES))
def test_hand_cases_through_the_pipe(gpu_scanner_factory, name):
    """The five hand cases of lanes_inputs: every frame under its own plane, against the hand-derived centres and the word
    of the hand-derived rose, under both reports, without a mask and under an all-ones one."""
    p, rows = pl.hand_rows(name)
    s = gpu_scanner_factory(p)
    ones = np.ones((p.grid_h, p.grid_w), dtype=bool)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        assert pipe.plane is None
        for f, (fr, plane, want_c, rose) in enumerate(rows):
            want = ([int(want_c >= 1)], [want_c], [direction.sector_word(rose)])
            assert both(pipe, [fr], plane) == want == pl.model(p, [fr], plane), (name, f)
            pipe.set_keep(ones)
            assert both(pipe, [fr], plane) == want, (name, f)
            pipe.set_keep(None)


def test_two_lanes_and_a_clock(gpu_scanner_factory):
    """pipe_lanes_inputs.two_lane_case(): 4 centres and the word of E 2 / S 2 / W 2 without the mask, 2 centres and the
    word of E 2 / W 2 with it.  No single byte gives these numbers."""
    p, fr, plane, keep, plain, masked = pl.two_lane_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        assert both(pipe, [fr], plane) == ([1], [plain[0]], [plain[1]])
        pipe.set_keep(keep)
        assert both(pipe, [fr], plane) == ([1], [masked[0]], [masked[1]])
        assert direction.unpack_sector_word(masked[1]) == (0x11, 0, 2)
        pipe.set_keep(np.ones((5, 6), dtype=bool))
        assert both(pipe, [fr], plane) == ([1], [plain[0]], [plain[1]])


# ------------------------------------------------------------------ 2. P1 - P6 in every layout and batch geometry

@pytest.fixture(scope="module")
def shapes_expected():
    """The model's answers for shapes_case(), once: {(plane name, masked): (flags, centres, words)}."""
    p, frames, keep, a, b = pl.shapes_case()
    planes = {"a": a, "b": b}
    planes.update({x: pl.filled(p, x) for x in pl.SHAPE_BYTES})
    want = {(n, k): pl.model(p, list(frames), pln, keep if k else None) for n, pln in planes.items() for k in (False, True)}
    return planes, want


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_p1_to_p6_in_every_layout_and_batch_geometry(gpu_scanner_factory, shapes_expected, layout):
    p, frames, keep, a, b = pl.shapes_case()
    planes, expected = shapes_expected
    frames = list(frames)
    s = gpu_scanner_factory(p)
    n = len(frames)
    ones = np.ones((p.grid_h, p.grid_w), dtype=bool)
    centres = bool(layout & CE)

    def pick(t):                                               # what a pipe of this layout can report
        return t if centres else (t[0], None, None)

    def scan(pipe, plane):
        if centres:
            return both(pipe, frames, plane)
        pipe.set_plane(plane)
        return run(pipe, frames) + (None,)

    def scan_dir(pipe, byte):
        if centres:
            return both_dir(pipe, frames, byte)
        pipe.clear_plane()
        pipe.set_dir(byte)
        out = run(pipe, frames) + (None,)
        pipe.clear_dir()
        return out

    geoms = [(8192, 1, 2), (8192, 4, 2), (16384, n, 2), (512, 5, 3)]          # one frame; 4; exactly the capacity; growing batches
    res_a = resident(s, frames, a)
    assert res_a == expected[("a", False)]
    kept = [None if f is None else pd.remove_masked(p, f, keep) for f in frames]
    assert resident_words(s, kept) == expected[("a", True)][2]
    for max_rec, max_fr, nbuf in geoms:
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout)) as pipe:
            plain = run(pipe, frames)
            pipe.set_keep(keep)
            masked = run(pipe, frames)
            pipe.set_keep(None)
            assert plain[0] == pg.masked_plain(p, frames)[0] and masked[0] == pg.masked_plain(p, frames, keep)[0]
            got_a = scan(pipe, a)                                  # P1: no keep plane == mtgpu_scan_frames_lanes, the word from its rose
            assert got_a == pick(res_a), max_fr
            pipe.set_keep(ones)                                    # P2: all ones == no keep plane
            assert scan(pipe, a) == pick(res_a), max_fr
            pipe.set_keep(keep)                                    # the model under the mask, both reports
            got_ak = scan(pipe, a)
            assert got_ak == pick(expected[("a", True)]), max_fr
            got_bk = scan(pipe, b)                                 # P6 and P5 under the mask
            assert got_bk == pick(expected[("b", True)]), max_fr
            if centres:
                assert all(y <= x for x, y in zip(got_ak[1], got_bk[1])) and got_ak[2] == got_bk[2]
            # P4: the masked pipe without the mode on the frames without their forbidden records
            pipe.clear_plane()
            assert pipe.plane is None
            assert run(pipe, pl.remove_forbidden(p, frames, a)) == (got_ak[0], got_ak[1]), max_fr
            pipe.set_keep(None)
            for byte in pl.SHAPE_BYTES:                            # P3: one byte everywhere == the direction pipe under it
                for k in (None, keep):
                    pipe.set_keep(k)
                    got = scan(pipe, planes[byte])
                    assert got == scan_dir(pipe, byte) == pick(expected[(byte, k is not None)]), (max_fr, byte)
                    if byte == 0xFF:
                        assert (got[0], got[1]) == (masked if k is not None else plain), max_fr
            pipe.set_keep(None)
            pipe.clear_plane()
            assert run(pipe, frames) == plain                      # plane == NULL: the plain pipe again
    with contextlib.closing(m.ScanPipe(s, 8192, 1, 1, layout=layout)) as pipe:         # one frame through a pipe of one batch
        pipe.set_keep(keep)
        pipe.set_plane(a, "sectors" if centres else "centres")
        want = expected[("a", True)]
        for i in (1, 7, 0, 5, 13):
            assert run(pipe, frames[i:i + 1]) == (want[0][i:i + 1], want[2][i:i + 1] if centres else None), i


# ------------------------------------------------------------------ 3. word seams and the byte phase of the staged copy

@pytest.mark.parametrize("margin", [0, 1], ids=["tail-byte", "head-bytes"])
@pytest.mark.parametrize("gw", [65, 129])
def test_word_seams_with_and_without_cleared_cells(gpu_scanner_factory, gw, margin):
    """lanes_inputs.seam_case(gw): bytes that change across 63 | 64 and 127 | 128.  margin 1: y_lo gw is odd, the staged
    copy starts three bytes in front of an aligned word; margin 0: one byte behind the last whole word."""
    fr, planes, hand = pl.seam_rows(gw)
    p = pl.seam_params(gw, margin)
    assert m.lanes_preview(p)["staged"] == 1
    s = gpu_scanner_factory(p)
    keep = pd.seam_keep(gw)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        for plane, c in zip(planes, hand):
            got = both(pipe, [fr], plane)
            assert got == pl.model(p, [fr], plane) and got[1] == [c], (gw, margin)
        pipe.set_keep(keep)
        for plane in planes:
            assert both(pipe, [fr], plane) == pl.model(p, [fr], plane, keep), (gw, margin)


# ------------------------------------------------------------------ 4. 4K: the unstaged and the staged form

@pytest.mark.parametrize("vertical_mask, staged", [(0.0, 0), (0.05, 1)], ids=["unstaged", "staged"])
@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC | CE, m.LAYOUT_AOS40 | CE], ids=["compact8-zero-copy", "aos40"])
def test_uhd_both_forms(gpu_scanner_factory, vertical_mask, staged, layout):
    p, frames, plane, keep = pl.uhd_rows(vertical_mask)
    frames = list(frames)
    assert m.lanes_preview(p)["staged"] == staged              # each form is known to have run
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, layout=layout)) as pipe:
        got = both(pipe, frames, plane)
        assert got == pl.model(p, frames, plane) == resident(s, frames, plane)
        pipe.set_keep(keep)
        assert both(pipe, frames, plane) == pl.model(p, frames, plane, keep)


# ------------------------------------------------------------------ 5. a frame in three pieces; the streamers' edges

def test_a_frame_of_three_pieces(gpu_scanner_factory):
    """300 000 records, compact: two whole pieces of the kernel's 131 072 and a third; the rose is flushed per piece and
    the word counts them all: 300 000, and 250 000 under the keep plane that clears the cell of every sixth record."""
    p, fr, half, full, keep = pl.pieces_rows()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, len(fr), 1, 1, centres=True)) as pipe:
        for masked in (False, True):
            pipe.set_keep(keep if masked else None)
            ce, wd = pl.PIECES_HAND[masked]
            for plane, c in zip((half, full), ce):
                assert both(pipe, [fr], plane) == ([1], [c], [wd]), masked
    assert direction.unpack_sector_word(pl.PIECES_HAND[True][1])[2] == 250000


@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC | CE, m.LAYOUT_AOS40 | CE], ids=["compact8-zero-copy", "aos40"])
def test_streamer_edges_through_the_pipe(gpu_scanner_factory, layout):
    """dir_inputs.edge_case(): every length of EDGE_LENGTHS on every 8-byte phase of a 128-byte line, in both record
    sizes, under the cell-wise plane; the padding frames have no side data and hold records that would show in a
    neighbour's rose."""
    e = di.edge_case()
    p, frames = e["params"], pd.case_frames(e)
    plane = li.cellwise_plane(p)
    live = [np.array(e["mv"][int(e["off"][f]):int(e["off"][f + 1])]) for f in range(len(frames))]
    s = gpu_scanner_factory(p)
    want = pl.model(p, frames, plane)
    assert [want[2][f] for f in e["test"]] == [direction.sector_word(e["hand_rose"][f]) for f in e["test"]]
    with contextlib.closing(m.ScanPipe(s, int(e["off"][-1]) + 16, len(frames), 2, layout=layout)) as pipe:
        pipe.set_plane(plane, "sectors")
        assert run(pipe, frames) == (want[0], want[2])
        pipe.set_plane(plane, "centres")
        assert run(pipe, frames) == (want[0], want[1])
        # every frame staged, the padding frames too, as frames with side data: their records move every test frame onto
        # the phase the case built it for, and a read outside a frame shows in its word
        wl = pl.model(p, live, plane)
        assert run(pipe, live) == (wl[0], wl[1])
        pipe.set_plane(plane, "sectors")
        got = run(pipe, live)
        assert got == (wl[0], wl[2]) and [got[1][f] for f in e["test"]] == [want[2][f] for f in e["test"]]


# ------------------------------------------------------------------ 6. the one exit: an empty analysed range, stale results

def raw_batch(lib, pipe, frames, plant=None):
    """One batch through the C ABI itself: acquire, add every frame, submit, collect -> (flags, counts) as lists.  plant:
    (flag byte, count word) written into the collected batch's result arrays — the pinned block's own memory, through the
    pointers the ABI hands out — before the batch is released: the next batch of a pipe of one buffer finds them there."""
    b = ctypes.c_void_p()
    assert lib.mtgpu_pipe_acquire(pipe._pipe, ctypes.byref(b)) == _abi.MT_OK
    for i, f in enumerate(frames):
        mv = np.ascontiguousarray(f, dtype=m.MV_DTYPE)
        assert lib.mtgpu_batch_add_frame(b, mv.ctypes.data_as(ctypes.c_void_p), mv.nbytes, 1, float(i), i) == _abi.MT_OK
    assert lib.mtgpu_pipe_submit(pipe._pipe, b) == _abi.MT_OK
    got, fl, n, ce = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_void_p()
    assert lib.mtgpu_pipe_collect(pipe._pipe, ctypes.byref(got), ctypes.byref(fl), None, None, ctypes.byref(n)) == _abi.MT_OK
    assert n.value == len(frames) and lib.mtgpu_batch_centres(got, ctypes.byref(ce)) == _abi.MT_OK
    flags = (ctypes.c_uint8 * n.value).from_address(fl.value)
    words = (ctypes.c_uint32 * n.value).from_address(ce.value)
    out = (list(flags), list(words))
    if plant is not None:
        for i in range(n.value):
            flags[i], words[i] = plant
    assert lib.mtgpu_pipe_release(pipe._pipe, got) == _abi.MT_OK
    return out


@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", ["centres", "sectors"])
def test_empty_analysed_range_stores_zeros_over_stale_values(gpu_scanner_factory, layout, report):
    """vertical_mask 0.5: no analysed row, frames with side data and moving records.  n_buffers = 1, zero-copy: the first
    batch's result arrays are overwritten by hand with flag 1 and a non-zero word; the second batch goes into the same
    slots, and the kernel's one exit — which an empty range reaches too — must store flag 0 and word 0 over them (the
    frames have side data: the planner does not answer them)."""
    p, frames = pl.empty_range_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    with contextlib.closing(m.ScanPipe(s, 4096, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_plane(pl.filled(p, 0xFF), report)
        assert raw_batch(lib, pipe, frames, plant=(1, 0xDEADBEEF)) == ([0] * 3, [0] * 3)
        assert raw_batch(lib, pipe, frames, plant=(1, 7)) == ([0] * 3, [0] * 3)
        pipe.set_keep(np.ones((p.grid_h, p.grid_w), dtype=bool))
        assert raw_batch(lib, pipe, frames) == ([0] * 3, [0] * 3)


@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", ["centres", "sectors"])
def test_no_stale_results_in_a_reused_pinned_block(gpu_scanner_factory, layout, report):
    """n_buffers = 1, zero-copy: batch 1 leaves flag 1 / 5 centres / the word of rose 2 / 2 / 1 in every slot of the pinned
    block; batch 2 goes into the same slots and every flag and word must read the new value — from the kernel's one
    exit, with and without a centre, and from the planning kernel.  Then quiet frames and frames without side data:
    every flag and word reads 0."""
    p, one, two, h1, h2 = pl.stale_case()
    s = gpu_scanner_factory(p)
    quiet = [np.zeros(0, dtype=m.MV_DTYPE), None, np.array(one[0][:0])]
    with contextlib.closing(m.ScanPipe(s, 64, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_plane(pl.filled(p, 0xFF), report)
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, two) == (h2["flags"], h2[report])
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, list(reversed(two))) == (list(reversed(h2["flags"])), list(reversed(h2[report])))
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, quiet) == ([0, 0, 0], [0, 0, 0])
        # a plane of zeros: the records count in the word and do not vote — flag 0, centres 0 over the stale 5s
        assert run(pipe, one) == (h1["flags"], h1[report])
        pipe.set_plane(pl.filled(p, 0x00), report)
        assert run(pipe, one) == ([0, 0, 0], [0, 0, 0] if report == "centres" else h1["sectors"])


# ------------------------------------------------------------------ 7. limits

@pytest.mark.parametrize("which", ["staged", "unstaged"])
def test_limit_shapes_of_the_plane_scan(gpu_scanner_factory, which):
    """The tallest 65-wide grid mtgpu_lanes_preview accepts staged, and the first it accepts only unstaged: equal to the
    model and the hand values, without a mask and (both lie below the masked scan's limit) with one."""
    gw, gh = pl.limit_shapes()[which]
    p = pl.limit_params(gw, gh)
    assert m.lanes_preview(p)["staged"] == (1 if which == "staged" else 0)
    s = gpu_scanner_factory(p)
    frames, keep = pl.limit_frames(gw, gh)
    frames, plane = list(frames), pl.limit_plane(gw, gh)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        for masked in (False, True):
            pipe.set_keep(keep if masked else None)
            got = both(pipe, frames, plane)
            assert got == pl.model(p, frames, plane, keep if masked else None), (which, masked)
            assert got == ([1, 1, 0],) + pl.LIMIT_HAND[masked], (which, masked)


def test_limit_shape_of_the_masked_scan_and_one_row_further(gpu_scanner_factory):
    """The tallest 65-wide grid of the masked scan: the mask is on there.  One row further set_keep is
    MT_ERR_UNSUPPORTED with the grid named, and the pipe goes on with the unmasked plane scan."""
    gw, gh = pl.limit_shapes()["masked"]
    for rows, masked in ((gh, True), (gh + 1, False)):
        p = pl.limit_params(gw, rows)
        s = gpu_scanner_factory(p)
        frames, keep = pl.limit_frames(gw, rows)
        frames, plane = list(frames), pl.limit_plane(gw, rows)
        with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
            pipe.set_plane(plane)
            if masked:
                pipe.set_keep(keep)
                assert pipe.has_keep
            else:
                with pytest.raises(m.MtgpuError) as e:
                    pipe.set_keep(keep)
                assert e.value.code == _abi.MT_ERR_UNSUPPORTED and f"{gw}x{rows}" in str(e.value)
                assert not pipe.has_keep and pipe.plane[1] == "centres" and np.array_equal(pipe.plane[0], plane)
                assert run(pipe, frames) == pl.model(p, frames, plane)[:2]      # the same pipe goes on, unmasked
            got = both(pipe, frames, plane)
            assert got == pl.model(p, frames, plane, keep if masked else None), rows
            assert got == ([1, 1, 0],) + pl.LIMIT_HAND[masked], rows


def test_row_banded_grid_is_unsupported(gpu_scanner_factory):
    """960 x 540 cells: set_plane is MT_ERR_UNSUPPORTED with the grid named, the setting stays off and the pipe goes on
    scanning plainly."""
    from mvtrim_amd import synth
    p = m.ScanParams.from_config(3840, 2160, **pl.FINE_KW)
    s = gpu_scanner_factory(p)
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        before = run(pipe, frames)[0]
        assert before == s.check_frames(m.FrameBatch.from_frames(frames)).tolist() == [0, 1, 1]
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_plane(np.full((540, 960), 0x01, dtype=np.uint8))
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.plane is None and m.load_library().mtgpu_pipe_plane(pipe._pipe, None, None) == 0
        assert run(pipe, frames)[0] == before


# ------------------------------------------------------------------ 8. contracts

def test_bad_arguments_change_nothing(gpu_scanner_factory):
    p, one, two, h1, h2 = pl.stale_case()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    south = pl.filled(p, 0x04)
    ptr = south.ctypes.data_as(ctypes.c_void_p)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2)) as pipe:                   # no MT_LAYOUT_CENTRES
        bad = [(_abi.MT_PIPE_REPORT_LARGEST, "report"), (_abi.MT_PIPE_REPORT_VECTOR, "report"), (4, "report"), (-1, "report"),
               (SEC, "MT_LAYOUT_CENTRES")]
        for state in (None, "centres"):
            if state:
                pipe.set_plane(south, state)
            for report, text in bad:
                assert lib.mtgpu_pipe_set_plane(pipe._pipe, ptr, report) == _abi.MT_ERR_INVALID, report
                assert text in lib.mtgpu_last_error().decode(), report
                assert (pipe.plane is None) if state is None else (pipe.plane[1] == state and np.array_equal(pipe.plane[0], south))
        assert lib.mtgpu_pipe_set_plane(None, ptr, 0) == _abi.MT_ERR_INVALID and lib.mtgpu_pipe_plane(None, None, None) == -1
        with pytest.raises(ValueError):
            pipe.set_plane(south, "vector")
        with pytest.raises(ValueError):
            pipe.set_plane(south.astype(np.int32))
        with pytest.raises(ValueError):
            pipe.set_plane(south.T)
        assert run(pipe, list(two))[0] == [0, 0, 0]                             # S alone: frame c's E and W records do not vote
        assert lib.mtgpu_pipe_set_plane(pipe._pipe, None, 77) == _abi.MT_OK and pipe.plane is None      # ignored at NULL
        r = ctypes.c_int(7)
        back = np.full((5, 6), 9, dtype=np.uint8)
        assert lib.mtgpu_pipe_plane(pipe._pipe, back.ctypes.data_as(ctypes.c_void_p), ctypes.byref(r)) == 0
        assert r.value == 7 and (back == 9).all()
        assert run(pipe, list(two))[0] == h2["flags"]
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        pipe.set_plane(south, "sectors")
        assert lib.mtgpu_pipe_plane(pipe._pipe, None, None) == 1 and pipe.plane[1] == "sectors"
        pipe.clear_plane()
        pipe.set_plane(south)                                                   # the report was reset at NULL
        assert pipe.plane[1] == "centres" and pipe.dir() is None and lib.mtgpu_pipe_dir(pipe._pipe, None, None) == 0


def test_busy_and_one_pipe_two_recordings(gpu_scanner_factory):
    p, frames, keep, a, b = pl.shapes_case()
    frames = list(frames)
    n = len(frames)
    s = gpu_scanner_factory(p)
    plain = pg.masked_plain(p, frames)
    wa = pl.model(p, frames, a)
    wb = pl.model(p, frames, b, keep)
    assert plain[1] != wa[1] != wb[1]
    with contextlib.closing(m.ScanPipe(s, 8192, 4, 3, centres=True)) as pipe:
        pipe.set_plane(a, "centres")
        assert run(pipe, frames) == (wa[0], wa[1])
        feed_all(pipe, frames[:3])                                              # a batch being filled (state 1)
        for call in (lambda: pipe.set_plane(b, "sectors"), pipe.clear_plane):
            with pytest.raises(m.MtgpuError) as e:
                call()
            assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value)
            assert pipe.plane[1] == "centres" and np.array_equal(pipe.plane[0], a)
        for i in range(3, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (wa[0], wa[1])
        feed_all(pipe, frames[:6])                                              # 4 submitted, 2 being filled
        pipe._submit()
        assert pipe._cur is None and pipe._inflight >= 1                        # in flight (state 2)
        with pytest.raises(m.MtgpuError) as e:
            pipe.clear_plane()
        assert e.value.code == _abi.MT_ERR_BUSY and "in flight" in str(e.value) and np.array_equal(pipe.plane[0], a)
        for i in range(6, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (wa[0], wa[1])
        # the next recording: another plane, the other report and a mask
        pipe.set_keep(keep)
        pipe.set_plane(b, "sectors")
        assert run(pipe, frames) == (wb[0], wb[2])
        pipe.clear_plane()
        assert run(pipe, frames) == pg.masked_plain(p, frames, keep)            # NULL: the masked pipe, bit for bit
        pipe.set_keep(None)
        assert run(pipe, frames) == plain


def test_keep_and_plane_commute(gpu_scanner_factory):
    p, frames, keep, a, b = pl.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    want, nomask = pl.model(p, frames, a, keep), pl.model(p, frames, a)
    results = []
    for order in ("keep-first", "plane-first"):
        with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, centres=True)) as pipe:
            if order == "keep-first":
                pipe.set_keep(keep)
                pipe.set_plane(a, "sectors")
            else:
                pipe.set_plane(a, "sectors")
                pipe.set_keep(keep)
            assert pipe.has_keep and pipe.plane[1] == "sectors"
            x = run(pipe, frames)
            pipe.set_keep(None)
            assert pipe.plane[1] == "sectors"
            results.append((x, run(pipe, frames)))
    assert results[0] == results[1] == ((want[0], want[2]), (nomask[0], nomask[2]))


def test_plane_and_the_scalar_direction_mode_refuse_each_other(gpu_scanner_factory):
    """One rule at two granularities: MT_ERR_INVALID both ways with the other setter named; nothing changes."""
    p, frames, keep, a, b = pl.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, centres=True)) as pipe:
        pipe.set_dir(0x5B, "sectors")
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_plane(a)
        assert e.value.code == _abi.MT_ERR_INVALID and "(mtgpu_pipe_set_dir)" in str(e.value)
        assert pipe.plane is None and pipe.dir() == (0x5B, "sectors")
        assert run(pipe, frames) == pd.model(p, frames, 0x5B)[::2]
        pipe.clear_plane()                                                      # off is always accepted
        assert pipe.dir() == (0x5B, "sectors")
        pipe.clear_dir()
        pipe.set_plane(a, "sectors")
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_dir(0x5B)
        assert e.value.code == _abi.MT_ERR_INVALID and "(mtgpu_pipe_set_plane)" in str(e.value)
        assert pipe.dir() is None and pipe.plane[1] == "sectors" and np.array_equal(pipe.plane[0], a)
        pipe.clear_dir()                                                        # off is always accepted
        assert run(pipe, frames) == pl.model(p, frames, a)[::2]


def test_plane_and_the_three_other_modes_refuse_each_other(gpu_scanner_factory):
    """All six refusals: MT_ERR_UNSUPPORTED with "not together yet" and the other setter named, both settings as they
    were; off is always accepted."""
    p, frames, keep, a, b = pl.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    others = [("mtgpu_pipe_set_blobs", lambda q: q.set_blobs(3, "largest"), lambda q: q.set_blobs(0), lambda q: q.blobs, (3, "largest")),
              ("mtgpu_pipe_set_gmc", lambda q: q.set_gmc(4, 100, "vector"), lambda q: q.clear_gmc(), lambda q: q.gmc(), (4, 100, "vector")),
              ("mtgpu_pipe_set_gmc_blobs", lambda q: q.set_gmc_blobs(2, 5, 90, "largest"), lambda q: q.clear_gmc_blobs(),
               lambda q: q.gmc_blobs(), (2, 5, 90, "largest"))]
    want = pl.model(p, frames, a)
    for setter, on, off, get, state in others:
        with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, centres=True)) as pipe:
            on(pipe)
            other_run = run(pipe, frames)
            with pytest.raises(m.MtgpuError) as e:
                pipe.set_plane(a, "sectors")
            assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value) and f"({setter})" in str(e.value)
            assert pipe.plane is None and get(pipe) == state
            pipe.clear_plane()                                                  # off is always accepted
            assert run(pipe, frames) == other_run
            off(pipe)
            pipe.set_plane(a, "sectors")
            with pytest.raises(m.MtgpuError) as e:
                on(pipe)
            assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value) and "(mtgpu_pipe_set_plane)" in str(e.value)
            assert get(pipe) is None and pipe.plane[1] == "sectors"
            off(pipe)                                                           # off is always accepted
            assert run(pipe, frames) == (want[0], want[2])
            pipe.clear_plane()
            on(pipe)
            assert run(pipe, frames) == other_run


def test_plane_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    p, one, two, h1, h2 = pl.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 64, 1, 2, centres=True)) as pipe:
        pipe.set_keep(np.ones((5, 6), dtype=bool))
        pipe.set_plane(pl.filled(p, 0xFF), "sectors")
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, list(one)) == (h1["flags"], h1["sectors"])    # three batches of one frame
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


# ------------------------------------------------------------------ 9. draws

@pytest.mark.parametrize("i", range(pl.N_DRAWS))
def test_draws_hold_p1_p2_p4_and_are_monotone(gpu_scanner_factory, i):
    p, frames, keep, chain = pl.draw(i)
    frames = list(frames)
    s = gpu_scanner_factory(p)
    ones = np.ones((p.grid_h, p.grid_w), dtype=bool)
    nrec = max(len(f) for f in frames if f is not None)
    layout = (m.LAYOUT_AOS40 if i % 2 else m.LAYOUT_COMPACT8) | (ZC if i % 4 < 2 else 0) | CE
    words = pl.sector_words(p, frames, keep)
    kept = [None if f is None else pd.remove_masked(p, f, keep) for f in frames]
    assert resident_words(s, kept) == words                     # P4, the word: the resident rose without the keep-0 records
    prev = None
    with contextlib.closing(m.ScanPipe(s, 2 * nrec, 5, 2, layout=layout)) as pipe:
        for j, plane in enumerate(chain):
            res = resident(s, frames, plane)
            assert both(pipe, frames, plane) == res, j          # P1
            pipe.set_keep(ones)
            assert both(pipe, frames, plane) == res, j          # P2
            pipe.set_keep(keep)
            got = both(pipe, frames, plane)
            assert got[2] == words, j                           # P5 along the chain
            if j in (1, 2, 3):
                assert got == pl.model(p, frames, plane, keep), j
            pipe.clear_plane()
            assert run(pipe, pl.remove_forbidden(p, frames, plane)) == (got[0], got[1]), j   # P4, the centres
            pipe.set_keep(None)
            assert prev is None or all(x <= y for x, y in zip(prev, got[1])), j      # P6 along the chain
            prev = got[1]
    assert got[:2] == pg.masked_plain(p, frames, keep)          # the chain ends at 0xFF: P3, against the model


# ------------------------------------------------------------------ 10. mtgpu_scan_file, the host layer, the example

MERGE_ENV = dict(MAX_GAP_SEC="0.2", PADDING_SEC="0.04", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="25")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 90-frame two-way road with its clock as a .mtmv file, the clock's mask as a .mtkeep file, and the inverted
    plane learned by `python -m mvtrim_amd.lanes --learn --save-plane` in a fresh child process as a .mtdir file."""
    d = tmp_path_factory.mktemp("pipe_lanes")
    p, frames, pts, keep, hand = pl.recording_case()
    path = str(d / "road.mtmv")
    m.mvfile.write_mtmv(path, 320, 160, 1, 25, pl.REC_FPS, pl.REC_FRAMES / pl.REC_FPS, list(range(pl.REC_FRAMES)), list(frames))
    mask = str(d / "clock.mtkeep")
    zones.save_keep(mask, keep)
    learned = str(d / "road.mtdir")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), PYTHONIOENCODING="utf-8")
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.lanes", path, "--mv-threshold-sq", "4", "--vectors-needed", "2",
                          "--clusters-needed", "1", "--vertical-mask", "0", "--learn", "--min-records", "4", "--share", "0.4",
                          "--widen", "1", "--save-plane", learned], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    plane = lanes.load_plane(learned, grid=(20, 10))
    assert np.array_equal(plane, hand)
    wrong = lanes.invert_plane(plane, plane != 0xFF, 0)
    wrong_path = str(d / "wrong_way.mtdir")
    lanes.save_plane(wrong_path, wrong)
    env = dict(os.environ, **MERGE_ENV, **pl.REC_ENV)
    for k in ("BLOCK_SIZE", "BLOCK_SHIFT", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, wrong_path, wrong, env


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=pl.REC_FRAMES / pl.REC_FPS, max_gap_sec=0.2, padding_sec=0.04, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def scan_file(env, path, *args):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2"] + list(args), capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def test_scan_file_plane_keep_and_sectors(gpu_scanner_factory, recording):
    path, mask, wrong_path, wrong, env = recording
    p, frames, pts, keep, _ = pl.recording_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    plain = scan_file(env, path)
    assert plain["motion_frames"] == pl.REC_FRAMES and "dir" not in plain
    # the Python path: the same plane and mask through a ScanPipe
    with contextlib.closing(m.ScanPipe(s, 4096, 16, 3, centres=True)) as pipe:
        pipe.set_keep(keep)
        pipe.set_plane(wrong, "sectors")
        py_fl, py_wd = run(pipe, frames, pts)
    fl, ce, wd = pl.model(p, frames, wrong, keep)
    assert (py_fl, py_wd) == (fl, wd) and [f for f in range(pl.REC_FRAMES) if fl[f]] == pl.AGAINST
    want_seg, want_res = python_segments(s, py_fl, pts)
    assert len(want_seg) == 2
    # without the mask the clock keeps every frame under the inverted plane
    r = scan_file(env, path, "--plane", wrong_path)
    assert r["motion_frames"] == pl.REC_FRAMES and r["segments"] == plain["segments"] and "dir" not in r
    r = scan_file(env, path, "--plane", wrong_path, "--keep", mask, "--timestamps")
    assert r["motion_frames"] == 20 and r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"]
    assert r["timestamps"] == [pts[f] for f in pl.AGAINST] and r["frames_scanned"] == pl.REC_FRAMES and r["ignored_cells"] == 3
    d = scan_file(env, path, "--plane", wrong_path, "--keep", mask, "--dir-sectors")
    fr_n, present, dominant = pl.recording_stats(wd)
    assert d["segments"] == want_seg and "centres" not in d
    assert d["dir"] == {"plane": wrong_path, "frames": fr_n, "present": present, "dominant": dominant} and fr_n == 60
    c = scan_file(env, path, "--plane", wrong_path, "--keep", mask, "--centres")
    assert [n for _, n in c["centres"]] == ce and c["segments"] == want_seg
    # persistence on the model's flags: both events are 10 frames long, --min-run 11 drops them
    r = scan_file(env, path, "--plane", wrong_path, "--keep", mask, "--min-run", "11")
    assert r["motion_frames"] == 0 and r["frames_before_persist"] == 20
    # a plane for another grid: the loader's message with the line named, status 1, no job printed
    other = os.path.join(os.path.dirname(wrong_path), "other.mtdir")
    lanes.save_plane(other, np.zeros((10, 21), dtype=np.uint8))
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2", "--plane", other], capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 1 and "--plane: " in out.stderr and "line 2" in out.stderr and "21x10" in out.stderr and out.stdout == ""


def test_next_video_does_not_inherit_the_plane(recording, tmp_path):
    """run_scan_pipeline on one pool of GpuBackends (tests/cpp/pipe_lanes_two_videos.cpp): the plane, plain, the plane with
    the sectors reported, and the plane together with dir_allow and with blobs, refused before any decode."""
    path, _, wrong_path, wrong, env = recording
    p, frames, pts, _, _ = pl.recording_case()
    frames = list(frames)
    exe = str(tmp_path / "pipe_lanes_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_lanes_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "2", wrong_path, "20", "10"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 5
    # no mask here: the clock votes under the inverted plane, every frame is kept; the plain run keeps every frame too
    under = pl.model(p, frames, wrong)
    want = [under, pg.masked_plain(p, frames) + ([0] * len(frames),), under]
    for i, r in enumerate(runs[:3]):
        kv = dict(zip(r[0::2], r[1::2]))
        fl, _, wd = want[i]
        ts = [float(t) for t in kv["timestamps"].split(",") if t != "-"]
        assert ts == [pts[f] for f in range(pl.REC_FRAMES) if fl[f]], i
        assert int(kv["motion_frames"]) == sum(fl) and int(kv["frames_scanned"]) == pl.REC_FRAMES
        assert kv["plane"].split(",") == [("1/0", "0/0", "1S/0")[i]] * 2
        if i == 2:
            fr_n, present, dominant = pl.recording_stats(wd)
            assert int(kv["frames"]) == fr_n == pl.REC_FRAMES
            assert kv["present"] == ":".join(map(str, present)) and kv["dominant"] == ":".join(map(str, dominant))
        else:
            assert kv["frames"] == "0" and kv["present"] == kv["dominant"] == "0:0:0:0:0:0:0:0"
    assert runs[3][:6] == ["run", "3", "rc", "1", "frames_scanned", "0"] and "one rule at two granularities" in " ".join(runs[3])
    assert runs[4][:6] == ["run", "4", "rc", "1", "frames_scanned", "0"] and "not together yet" in " ".join(runs[4])
    assert "dir_plane" in " ".join(runs[3]) and "dir_allow" in " ".join(runs[3])
    assert "dir_plane" in " ".join(runs[4]) and "min_blob_cells" in " ".join(runs[4])


def test_plain_c_pipe_lanes_example(tmp_path):
    exe = str(tmp_path / "pipe_lanes_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_lanes_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0xFF everywhere              20 frames kept, 2 segment(s)" in out.stdout
    assert "upper half: not E, NE, SE    10 frames kept, 1 segment(s)" in out.stdout
