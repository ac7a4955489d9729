"""GPU tier (`-m gpu`): the direction filter carried through the pipe under its keep mask (include/mtgpu_pipe_dir.h;
csrc/dir_kernels.hip, the pipe form), the C++ host layer and mtgpu_scan_file.  Expected values: numbers derived by hand
and the model (tests/pipe_dir_inputs.py; both checked without a GPU by tests/test_pipe_dir_host.py), and
mtgpu_scan_frames_dir / the plain and the masked pipe on the same frames for D1 - D5.  Every comparison is exact."""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, zones

import dir_inputs as di
import persist_model as pm
import pipe_dir_inputs as pd
import pipe_gmc_inputs as pg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES
LAYOUTS = [rec | zc | CE for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC)]
LAYOUT_IDS = ["-".join([r] + z) for r in ("compact8", "aos40") for z in ([], ["zero-copy"])]
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


def both(pipe, frames, allow):
    """(flags, centres, words) of a pipe with MT_LAYOUT_CENTRES under `allow`: one run per report; the flags agree."""
    pipe.set_dir(allow, "centres")
    assert pipe.dir() == (allow, "centres")
    fl, ce = run(pipe, frames)
    pipe.set_dir(allow, "sectors")
    assert pipe.dir() == (allow, "sectors")
    fl2, wd = run(pipe, frames)
    assert fl == fl2
    return fl, ce, wd


def resident(s, frames, allow):
    """mtgpu_scan_frames_dir with the scalar allow on the same frames -> (flags, centres, words derived from its rose)."""
    r = s.scan_dir(m.FrameBatch.from_frames(list(frames)), allow)
    return r["flags"].tolist(), r["centres"].tolist(), [direction.sector_word(x) for x in r["rose"].tolist()]


# ------------------------------------------------------------------ 1. the hand cases through the pipe

@pytest.mark.parametrize("name", list(di.HAND_CASES))
def test_hand_cases_through_the_pipe(gpu_scanner_factory, name):
    """The four hand cases of dir_inputs: every frame under its stream's byte, against the hand-derived centres and the
    word of the hand-derived rose.  boundary: 5, 0, 4, 0, 2, 0 and the word of rose 2 / 2 / 1 under every byte (D5);
    vn0: the plain count whatever the byte."""
    case = di.HAND_CASES[name]()
    p, frames, allows = case["params"], pd.case_frames(case), pd.case_allows(case)
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        assert pipe.dir() is None
        for f, (fr, a) in enumerate(zip(frames, allows)):
            want_c, want_w = int(case["hand_centres"][f]), direction.sector_word(case["hand_rose"][f])
            assert both(pipe, [fr], a) == ([int(want_c >= 1)], [want_c], [want_w]) == pd.model(p, [fr], a), (name, f)
        if name == "boundary":
            assert [both(pipe, frames[:1], a)[1:] for a in di.BOUNDARY_ALLOWS] == [([c], [pd.BOUNDARY_WORD]) for c in (5, 0, 4, 0, 2, 0)]
        if name == "vn0":
            pipe.clear_dir()
            plain = run(pipe, frames)
            assert plain[1] == [20, 20, 20]
            for a in (0x00, 0x10, 0xFF):
                assert both(pipe, frames, a)[:2] == plain


# ------------------------------------------------------------------ 2. hand frames under a mask

def test_the_mask_reaches_the_rose_and_the_active_plane(gpu_scanner_factory):
    """pipe_dir_inputs.mask_hand().  Frame a fails on a build whose mask reaches only the active plane: its word would
    read dominant E, count 6."""
    for name, (p, fr, keep, allow, masked, plain) in pd.mask_hand().items():
        s = gpu_scanner_factory(p)
        with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
            fl, ce, wd = both(pipe, [fr], allow)
            assert (ce[0], wd[0]) == plain and fl == [int(plain[0] >= 1)], name
            pipe.set_keep(keep)
            fl, ce, wd = both(pipe, [fr], allow)
            assert (ce[0], wd[0]) == masked and fl == [int(masked[0] >= 1)], name
            if name == "a":
                assert direction.unpack_sector_word(wd[0]) == (0x10, 4, 2)
            pipe.set_keep(np.ones((5, 6), dtype=bool))
            assert both(pipe, [fr], allow)[1:] == ([plain[0]], [plain[1]]), name


# ------------------------------------------------------------------ 3. D1 - D4 in every layout and batch geometry

@pytest.fixture(scope="module")
def shapes_expected():
    """The model's answers for shapes_case(), once: {(allow, masked): (flags, centres, words)}."""
    p, frames, keep = pd.shapes_case()
    return {(a, k): pd.model(p, list(frames), a, keep if k else None) for a in pd.SHAPE_ALLOWS for k in (False, True)}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_d1_to_d4_in_every_layout_and_batch_geometry(gpu_scanner_factory, shapes_expected, layout):
    p, frames, keep = pd.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    n = len(frames)
    ones = np.ones((p.grid_h, p.grid_w), dtype=bool)
    geoms = [(8192, 1, 2), (8192, 4, 2), (16384, n, 2), (512, 5, 3)]          # one frame; 4; exactly the capacity; growing batches
    for max_rec, max_fr, nbuf in geoms:
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout)) as pipe:
            plain = run(pipe, frames)
            pipe.set_keep(keep)
            masked = run(pipe, frames)
            pipe.set_keep(None)
            assert plain == pg.masked_plain(p, frames) and masked == pg.masked_plain(p, frames, keep)
            for a in pd.SHAPE_ALLOWS:
                want, wantk = shapes_expected[(a, False)], shapes_expected[(a, True)]
                res = resident(s, frames, a)
                assert res == want, a
                got = both(pipe, frames, a)                   # D1: no keep plane == mtgpu_scan_frames_dir, the word from its rose
                assert got == res, (max_fr, a)
                pipe.set_keep(ones)                           # D2: all ones == no keep plane
                assert both(pipe, frames, a) == res, (max_fr, a)
                pipe.set_keep(keep)                           # the model under the mask, both reports
                gotk = both(pipe, frames, a)
                assert gotk == wantk, (max_fr, a)
                # D4: the masked pipe without the mode on the frames without their forbidden records; the resident rose of
                # the frames without their keep-0 records
                pipe.clear_dir()
                assert pipe.dir() is None
                allowed = [None if f is None else pd.remove_forbidden(f, a) for f in frames]
                assert run(pipe, allowed) == (gotk[0], gotk[1]), (max_fr, a)
                kept = [None if f is None else pd.remove_masked(p, f, keep) for f in frames]
                assert resident(s, kept, 0xFF)[2] == gotk[2], (max_fr, a)
                if a == 0xFF:                                 # D3: every sector allowed == the pipe without the mode
                    assert (gotk[0], gotk[1]) == masked and (got[0], got[1]) == plain
                pipe.set_keep(None)
            assert run(pipe, frames) == plain                 # enable == 0: the plain pipe again
    with contextlib.closing(m.ScanPipe(s, 8192, 1, 1, layout=layout)) as pipe:         # one frame through a pipe of one batch
        pipe.set_keep(keep)
        pipe.set_dir(0x5B, "sectors")
        wantk = shapes_expected[(0x5B, True)]
        for i in (1, 7, 0, 5):
            assert run(pipe, frames[i:i + 1]) == (wantk[0][i:i + 1], wantk[2][i:i + 1]), i


# ------------------------------------------------------------------ 4. the streamers' edges

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC | CE, m.LAYOUT_AOS40 | CE], ids=["compact8-zero-copy", "aos40"])
def test_streamer_edges_through_the_pipe(gpu_scanner_factory, layout):
    """dir_inputs.edge_case(): every length of EDGE_LENGTHS on every 8-byte phase of a 128-byte line, in both record
    sizes; the padding frames have no side data and hold records that would show in a neighbour's rose."""
    e = di.edge_case()
    p, frames = e["params"], pd.case_frames(e)
    live = [np.array(e["mv"][int(e["off"][f]):int(e["off"][f + 1])]) for f in range(len(frames))]
    s = gpu_scanner_factory(p)
    want = pd.model(p, frames, di.EDGE_ALLOW)
    assert [want[2][f] for f in e["test"]] == [direction.sector_word(e["hand_rose"][f]) for f in e["test"]]
    with contextlib.closing(m.ScanPipe(s, int(e["off"][-1]) + 16, len(frames), 2, layout=layout)) as pipe:
        # as the case stands: a pipe stages nothing for a frame without side data, so the planner answers the padding frames
        pipe.set_dir(di.EDGE_ALLOW, "sectors")
        fl, wd = run(pipe, frames)
        assert (fl, wd) == (want[0], want[2])
        pipe.set_dir(di.EDGE_ALLOW, "centres")
        assert run(pipe, frames) == (want[0], want[1])
        # every frame staged, the padding frames too, as frames with side data: their records move every test frame onto
        # the phase the case built it for, and a read outside a frame shows in its word
        wl = pd.model(p, live, di.EDGE_ALLOW)
        assert run(pipe, live) == (wl[0], wl[1])
        pipe.set_dir(di.EDGE_ALLOW, "sectors")
        got = run(pipe, live)
        assert got == (wl[0], wl[2]) and [got[1][f] for f in e["test"]] == [want[2][f] for f in e["test"]]


@pytest.mark.parametrize("gw", [65, 129])
def test_word_seams_with_and_without_cleared_cells(gpu_scanner_factory, gw):
    case = di.seam_case(gw)
    p, fr = case["params"], pd.case_frames(case)[0]
    s = gpu_scanner_factory(p)
    rose_word = direction.sector_word(case["hand_rose"][0])
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        for a, c in zip(di.SEAM_ALLOWS, di.SEAM_HAND[gw]):
            assert both(pipe, [fr], a) == ([int(c >= 1)], [c], [rose_word]), a
        keep = pd.seam_keep(gw)
        pipe.set_keep(keep)
        for a, c in zip(di.SEAM_ALLOWS, pd.SEAM_MASKED_HAND[gw]):
            assert both(pipe, [fr], a) == ([int(c >= 1)], [c], pd.sector_words(p, [fr], keep)), a


def test_a_frame_of_three_pieces(gpu_scanner_factory):
    """262 145 records, compact: two whole pieces of kDirChunk and one record; the bulk in one sector, one record in each
    other: count 262 138, present 0xFF."""
    p, big = pd.big_case()
    s = gpu_scanner_factory(p)
    want = pd.model(p, [big], 0xF7)
    assert want[2] == [pd.BIG_WORD] and direction.unpack_sector_word(pd.BIG_WORD) == (0xFF, 3, 262138)
    with contextlib.closing(m.ScanPipe(s, len(big), 1, 1, centres=True)) as pipe:
        assert both(pipe, [big], 0xF7) == want


# ------------------------------------------------------------------ 5. stale results in the pinned block

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", ["centres", "sectors"])
def test_no_stale_results_in_a_reused_pinned_block(gpu_scanner_factory, layout, report):
    """n_buffers = 1, zero-copy: batch 1 leaves flag 1 / 5 centres / the word of rose 2 / 2 / 1 in every slot of the pinned
    block; batch 2 goes into the same slots and every flag and word must read the new value — from the kernel's one
    exit, with and without a centre, and from the planning kernel."""
    p, one, two, h1, h2 = pd.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 64, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_dir(0xFF, report)
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, two) == (h2["flags"], h2[report])
        assert run(pipe, one) == (h1["flags"], h1[report])
        assert run(pipe, list(reversed(two))) == (list(reversed(h2["flags"])), list(reversed(h2[report])))


# ------------------------------------------------------------------ 6. limits

def _limit_run(s, shape, keep):
    frames = list(pd.limit_frames(*shape)[0])
    out = []
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        if keep is not None:
            pipe.set_keep(keep)
        for a in pd.LIMIT_ALLOWS:
            out.append(both(pipe, frames, a))
    return frames, out


def test_limit_shape_only_the_direction_scan_accepts(gpu_scanner_factory):
    """The tallest 65-wide grid of mtgpu_dir_preview, which mtgpu_zones_preview rejects: set_dir is OK, set_keep is
    MT_ERR_UNSUPPORTED with the grid named, and the pipe runs unmasked direction equal to the model and the hand values."""
    gw, gh = pd.limit_shape()
    p = pd.limit_params(gw, gh)
    s = gpu_scanner_factory(p)
    frames = list(pd.limit_frames(gw, gh)[0])
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        pipe.set_dir(0x05)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_keep(np.ones((gh, gw), dtype=bool))
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and f"{gw}x{gh}" in str(e.value)
        assert not pipe.has_keep and pipe.dir() == (0x05, "centres")
        # the same pipe goes on: unmasked direction, first under the byte it had when the mask was refused
        assert run(pipe, frames) == pd.model(p, frames, 0x05)[:2] == ([1, 0, 0], pd.LIMIT_HAND[False][0][1])
        for a, ce in zip(pd.LIMIT_ALLOWS, pd.LIMIT_HAND[False][0]):
            got = both(pipe, frames, a)
            assert got == pd.model(p, frames, a) and got[1:] == (ce, pd.LIMIT_HAND[False][1]), a


def test_limit_shape_of_the_masked_scan(gpu_scanner_factory):
    """The tallest 65-wide grid of the masked scan: masked direction runs there and equals the model and the hand values."""
    shape = pd.masked_limit_shape()
    p = pd.limit_params(*shape)
    s = gpu_scanner_factory(p)
    keep = pd.limit_frames(*shape)[1]
    frames, out = _limit_run(s, shape, keep)
    for a, got, ce in zip(pd.LIMIT_ALLOWS, out, pd.LIMIT_HAND[True][0]):
        assert got == pd.model(p, frames, a, keep) and got[1:] == (ce, pd.LIMIT_HAND[True][1]), a


def test_row_banded_grid_is_unsupported(gpu_scanner_factory):
    """960 x 540 cells: set_dir is MT_ERR_UNSUPPORTED with the grid named, the setting stays off and the pipe goes on
    scanning plainly."""
    from mvtrim_amd import synth
    p = m.ScanParams.from_config(3840, 2160, **pd.FINE_KW)
    s = gpu_scanner_factory(p)
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        before = run(pipe, frames)[0]
        assert before == s.check_frames(m.FrameBatch.from_frames(frames)).tolist() == [0, 1, 1]
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_dir(0x01)
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.dir() is None and m.load_library().mtgpu_pipe_dir(pipe._pipe, None, None) == 0
        assert run(pipe, frames)[0] == before


# ------------------------------------------------------------------ 7. contracts

def test_bad_arguments_change_nothing(gpu_scanner_factory):
    p, one, two, h1, h2 = pd.stale_case()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2)) as pipe:                   # no MT_LAYOUT_CENTRES
        bad = [((1, -1, 0), "allow"), ((1, 256, 0), "allow"), ((1, 0xFF, _abi.MT_PIPE_REPORT_LARGEST), "report"),
               ((1, 0xFF, _abi.MT_PIPE_REPORT_VECTOR), "report"), ((1, 0xFF, 4), "report"), ((1, 0xFF, -1), "report"),
               ((1, 0xFF, SEC), "MT_LAYOUT_CENTRES")]
        for state in (None, (0x04, "centres")):
            if state:
                pipe.set_dir(*state)
            for args, word in bad:
                assert lib.mtgpu_pipe_set_dir(pipe._pipe, *args) == _abi.MT_ERR_INVALID, args
                assert word in lib.mtgpu_last_error().decode(), args
                assert pipe.dir() == state
        assert lib.mtgpu_pipe_set_dir(None, 1, 0xFF, 0) == _abi.MT_ERR_INVALID and lib.mtgpu_pipe_dir(None, None, None) == -1
        with pytest.raises(ValueError):
            pipe.set_dir(0xFF, "vector")
        assert run(pipe, list(two))[0] == [0, 0, 0]                             # S alone: frame c's E and W records do not vote
        assert lib.mtgpu_pipe_set_dir(pipe._pipe, 0, 999, 77) == _abi.MT_OK and pipe.dir() is None     # ignored at enable 0
        a, c = ctypes.c_int32(7), ctypes.c_int(7)
        assert lib.mtgpu_pipe_dir(pipe._pipe, ctypes.byref(a), ctypes.byref(c)) == 0 and (a.value, c.value) == (7, 7)
        assert run(pipe, list(two))[0] == h2["flags"]
        pipe.set_dir(["E", "se"])                                               # names through direction.allow_from_names
        assert pipe.dir() == (0x03, "centres")
        pipe.set_dir("W,NW,SW")
        assert pipe.dir() == (0x38, "centres")
    with contextlib.closing(m.ScanPipe(s, 64, 2, 2, centres=True)) as pipe:
        pipe.set_dir(0x11, "sectors")
        assert lib.mtgpu_pipe_dir(pipe._pipe, None, None) == 1 and pipe.dir() == (0x11, "sectors")
        pipe.clear_dir()
        pipe.set_dir()                                                          # the report was reset at enable 0
        assert pipe.dir() == (0xFF, "centres")


def test_busy_and_one_pipe_two_recordings(gpu_scanner_factory):
    p, frames, keep = pd.shapes_case()
    frames = list(frames)
    n = len(frames)
    s = gpu_scanner_factory(p)
    plain = pg.masked_plain(p, frames)
    a = pd.model(p, frames, 0x5B)
    b = pd.model(p, frames, 0x01, keep)
    assert plain[1] != a[1] != b[1]
    with contextlib.closing(m.ScanPipe(s, 8192, 4, 3, centres=True)) as pipe:
        pipe.set_dir(0x5B, "centres")
        assert run(pipe, frames) == (a[0], a[1])
        feed_all(pipe, frames[:3])                                              # a batch being filled
        for call in (lambda: pipe.set_dir(0x01, "sectors"), pipe.clear_dir):
            with pytest.raises(m.MtgpuError) as e:
                call()
            assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value) and pipe.dir() == (0x5B, "centres")
        for i in range(3, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (a[0], a[1])
        feed_all(pipe, frames[:6])                                              # 4 submitted, 2 being filled
        pipe._submit()
        assert pipe._cur is None and pipe._inflight >= 1
        with pytest.raises(m.MtgpuError) as e:
            pipe.clear_dir()
        assert e.value.code == _abi.MT_ERR_BUSY and "in flight" in str(e.value) and pipe.dir() == (0x5B, "centres")
        for i in range(6, n):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == (a[0], a[1])
        # the next recording: another byte, the other report and a mask
        pipe.set_keep(keep)
        pipe.set_dir(0x01, "sectors")
        assert run(pipe, frames) == (b[0], b[2])
        pipe.clear_dir()
        assert run(pipe, frames) == pg.masked_plain(p, frames, keep)            # enable == 0: the masked pipe, bit for bit
        pipe.set_keep(None)
        assert run(pipe, frames) == plain


def test_keep_and_dir_commute(gpu_scanner_factory):
    p, frames, keep = pd.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    want, nomask = pd.model(p, frames, 0x5B, keep), pd.model(p, frames, 0x5B)
    results = []
    for order in ("keep-first", "dir-first"):
        with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, centres=True)) as pipe:
            if order == "keep-first":
                pipe.set_keep(keep)
                pipe.set_dir(0x5B, "sectors")
            else:
                pipe.set_dir(0x5B, "sectors")
                pipe.set_keep(keep)
            assert pipe.has_keep and pipe.dir() == (0x5B, "sectors")
            x = run(pipe, frames)
            pipe.set_keep(None)
            assert pipe.dir() == (0x5B, "sectors")
            results.append((x, run(pipe, frames)))
    assert results[0] == results[1] == ((want[0], want[2]), (nomask[0], nomask[2]))


def test_direction_and_the_three_other_modes_refuse_each_other(gpu_scanner_factory):
    """All six refusals: MT_ERR_UNSUPPORTED with "not together yet" and the other setter named, both settings as they
    were; off is always accepted."""
    p, frames, _ = pd.shapes_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    others = [("mtgpu_pipe_set_blobs", lambda q: q.set_blobs(3, "largest"), lambda q: q.set_blobs(0), lambda q: q.blobs, (3, "largest")),
              ("mtgpu_pipe_set_gmc", lambda q: q.set_gmc(4, 100, "vector"), lambda q: q.clear_gmc(), lambda q: q.gmc(), (4, 100, "vector")),
              ("mtgpu_pipe_set_gmc_blobs", lambda q: q.set_gmc_blobs(2, 5, 90, "largest"), lambda q: q.clear_gmc_blobs(),
               lambda q: q.gmc_blobs(), (2, 5, 90, "largest"))]
    want = pd.model(p, frames, 0x1B)
    for setter, on, off, get, state in others:
        with contextlib.closing(m.ScanPipe(s, 8192, 4, 2, centres=True)) as pipe:
            on(pipe)
            other_run = run(pipe, frames)
            with pytest.raises(m.MtgpuError) as e:
                pipe.set_dir(0x1B, "sectors")
            assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value) and f"({setter})" in str(e.value)
            assert pipe.dir() is None and get(pipe) == state
            pipe.clear_dir()                                                    # off is always accepted
            assert run(pipe, frames) == other_run
            off(pipe)
            pipe.set_dir(0x1B, "sectors")
            with pytest.raises(m.MtgpuError) as e:
                on(pipe)
            assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value) and "(mtgpu_pipe_set_dir)" in str(e.value)
            assert get(pipe) is None and pipe.dir() == (0x1B, "sectors")
            off(pipe)                                                           # off is always accepted
            assert run(pipe, frames) == (want[0], want[2])
            pipe.clear_dir()
            on(pipe)
            assert run(pipe, frames) == other_run


def test_dir_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    p, one, two, h1, h2 = pd.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 64, 1, 2, centres=True)) as pipe:
        pipe.set_keep(np.ones((5, 6), dtype=bool))
        pipe.set_dir(0xFF, "sectors")
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, list(one)) == (h1["flags"], h1["sectors"])    # three batches of one frame
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


# ------------------------------------------------------------------ 8. draws

@pytest.mark.parametrize("i", range(pd.N_DRAWS))
def test_draws_hold_d1_d2_d4_and_are_monotone(gpu_scanner_factory, i):
    p, frames, keep = pd.draw(i)
    frames = list(frames)
    s = gpu_scanner_factory(p)
    ones = np.ones((p.grid_h, p.grid_w), dtype=bool)
    nrec = max(len(f) for f in frames if f is not None)
    layout = (m.LAYOUT_AOS40 if i % 2 else m.LAYOUT_COMPACT8) | (ZC if i % 4 < 2 else 0) | CE
    words = pd.sector_words(p, frames, keep)
    kept = [None if f is None else pd.remove_masked(p, f, keep) for f in frames]
    assert resident(s, kept, 0xFF)[2] == words                  # D4, the word: the resident rose without the keep-0 records
    prev = None
    with contextlib.closing(m.ScanPipe(s, 2 * nrec, 5, 2, layout=layout)) as pipe:
        for a in pd.DRAW_ALLOWS:
            res = resident(s, frames, a)
            assert both(pipe, frames, a) == res, a              # D1
            pipe.set_keep(ones)
            assert both(pipe, frames, a) == res, a              # D2
            pipe.set_keep(keep)
            got = both(pipe, frames, a)
            assert got[2] == words, a                           # D5 along the chain
            pipe.clear_dir()
            allowed = [None if f is None else pd.remove_forbidden(f, a) for f in frames]
            assert run(pipe, allowed) == (got[0], got[1]), a    # D4, the centres: the masked pipe without the forbidden records
            pipe.set_keep(None)
            assert prev is None or all(x <= y for x, y in zip(prev, got[1])), a      # monotone along the chain
            prev = got[1]
    assert got[:2] == pg.masked_plain(p, frames, keep)          # the chain ends at 0xFF: D3, against the model


# ------------------------------------------------------------------ 9. mtgpu_scan_file, the host layer, the example

MERGE_ENV = dict(MAX_GAP_SEC="0.1", PADDING_SEC="0.04", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="25")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 40-frame recording with its clock as a .mtmv file, the clock's mask as a .mtkeep file."""
    d = tmp_path_factory.mktemp("pipe_dir")
    p, frames, pts, keep = pd.recording_case()
    path = str(d / "street.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, pd.REC_FPS, pd.REC_FRAMES / pd.REC_FPS, list(range(pd.REC_FRAMES)), list(frames))
    mask = str(d / "clock.mtkeep")
    zones.save_keep(mask, keep)
    env = dict(os.environ, **MERGE_ENV)
    for k in ("CLUSTERS_NEEDED", "VECTORS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, env


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=pd.REC_FRAMES / pd.REC_FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def scan_file(env, path, *args):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2"] + list(args), capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    d = json.loads(out.stdout)
    # the first value: the printed keys and values in their order, without the wall times (every key that ends in _us)
    return [(k, v) for k, v in d.items() if not k.endswith("_us")], d


def test_scan_file_allow_ignore_keep_and_sectors(gpu_scanner_factory, recording):
    path, mask, env = recording
    p, frames, pts, keep = pd.recording_case()
    frames = list(frames)
    s = gpu_scanner_factory(p)
    plain_text, plain = scan_file(env, path)
    assert plain["motion_frames"] == 38 and "dir" not in plain
    assert scan_file(env, path, "--min-blob-cells", "0")[0] == plain_text       # none of the three options: the same output
    east_allow, west_allow = direction.allow_from_names("E,SE,S,N,NE"), direction.allow_from_names("S,SW,W,NW,N")
    for ignore, allow, event in (("W,NW,SW", east_allow, pd.EAST), ("E,NE,SE", west_allow, pd.WEST)):
        # without the mask the clock keeps every frame; under it the event's frames remain
        if event is pd.EAST:
            _, r = scan_file(env, path, "--ignore", ignore)
            assert r["motion_frames"] == 38 and r["segments"] == plain["segments"] and "dir" not in r
        fl, ce, wd = pd.model(p, frames, allow, keep)
        assert [f for f in range(pd.REC_FRAMES) if fl[f]] == list(event)
        want_seg, want_res = python_segments(s, fl, pts)
        text, r = scan_file(env, path, "--ignore", ignore, "--keep", mask)
        assert r["motion_frames"] == len(event) and r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"], ignore
        assert r["frames_scanned"] == pd.REC_FRAMES and "ignored_cells" in r and "dir" not in r
        names = direction.names_from_allow(allow)
        # --allow with the complement, as names and as a number
        assert scan_file(env, path, "--allow", names if event is pd.EAST else str(allow), "--keep", mask)[0] == text
        if event is pd.WEST:
            _, c = scan_file(env, path, "--ignore", ignore, "--keep", mask, "--centres")
            assert [n for _, n in c["centres"]] == ce and c["segments"] == want_seg
        _, d = scan_file(env, path, "--ignore", ignore, "--keep", mask, "--dir-sectors")
        fr_n, present, dominant = pd.recording_stats(wd)
        assert d["segments"] == want_seg and "centres" not in d
        assert d["dir"] == {"allow": allow, "frames": fr_n, "present": present, "dominant": dominant}
    # --dir-sectors alone implies the mode with every sector allowed
    _, d = scan_file(env, path, "--dir-sectors")
    fr_n, present, dominant = pd.recording_stats(pd.sector_words(p, frames))
    assert d["segments"] == plain["segments"] and d["dir"] == {"allow": 255, "frames": fr_n, "present": present, "dominant": dominant}
    assert fr_n == 38 and present[2] == 38
    # persistence on the model's flags: the west event (6 frames) falls to --min-run 8, the east one (10) stays
    for allow, want_n in ((0xFF, 10), (west_allow, 0)):
        fl = pd.model(p, frames, allow, keep)[0]
        sd = np.array([f is not None for f in frames], dtype=np.uint8)
        kept = pm.persist(fl, [0, pd.REC_FRAMES], sd, min_run=8, max_dropout=0)["flags"]
        assert int(kept.sum()) == want_n
        _, r = scan_file(env, path, "--allow", str(allow), "--keep", mask, "--min-run", "8")
        assert r["motion_frames"] == want_n and r["segments"] == python_segments(s, kept, pts)[0] and r["frames_before_persist"] == sum(fl)
    # usage errors: one line, status 2, nothing decoded
    exe = os.path.join(PKG, "mtgpu_scan_file")
    for args, text in ((["--allow", "E", "--ignore", "W"], "--allow cannot be combined with --ignore"),
                       (["--allow", "E", "--gmc"], "--allow cannot be combined with --gmc"),
                       (["--ignore", "E", "--min-blob-cells", "3"], "--ignore cannot be combined with --min-blob-cells"),
                       (["--dir-sectors", "--centres"], "--dir-sectors cannot be combined with --centres"),
                       (["--allow", "EAST"], "--allow takes a comma-separated list of sector names")):
        out = subprocess.run([exe, path, "--threads", "2"] + args, capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 2 and text in out.stderr and out.stdout == "", (args, out.stderr)


def test_next_video_does_not_inherit_the_dir_setting(recording, tmp_path):
    """run_scan_pipeline on one pool of GpuBackends (tests/cpp/pipe_dir_two_videos.cpp): direction, plain, another byte
    with the sectors reported, and direction together with blobs, refused before any decode."""
    path, _, env = recording
    p, frames, pts, _ = pd.recording_case()
    frames = list(frames)
    exe = str(tmp_path / "pipe_dir_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_dir_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 4
    # no mask here: the clock moves south.  0xC7 allows S: every frame; 0x7C allows S too; the plain run: every frame
    want = [pd.model(p, frames, 0xC7), pg.masked_plain(p, frames) + ([0] * len(frames),), pd.model(p, frames, 0x7C)]
    for i, r in enumerate(runs[:3]):
        kv = dict(zip(r[0::2], r[1::2]))
        fl, _, wd = want[i]
        ts = [float(t) for t in kv["timestamps"].split(",") if t != "-"]
        assert ts == [pts[f] for f in range(pd.REC_FRAMES) if fl[f]], i
        assert int(kv["motion_frames"]) == sum(fl) and int(kv["frames_scanned"]) == pd.REC_FRAMES
        assert kv["dir"].split(",") == [("199", "-1", "124S")[i]] * 2
        if i == 2:
            fr_n, present, dominant = pd.recording_stats(wd)
            assert int(kv["frames"]) == fr_n == 38
            assert kv["present"] == ":".join(map(str, present)) and kv["dominant"] == ":".join(map(str, dominant))
            assert present[0] == 10 and present[4] == 6 and dominant[2] == 38
        else:
            assert kv["frames"] == "0" and kv["present"] == kv["dominant"] == "0:0:0:0:0:0:0:0"
    assert runs[3][:6] == ["run", "3", "rc", "1", "frames_scanned", "0"] and "not together yet" in " ".join(runs[3])
    assert "dir_allow" in " ".join(runs[3]) and "min_blob_cells" in " ".join(runs[3])


def test_plain_c_pipe_dir_example(tmp_path):
    exe = str(tmp_path / "pipe_dir_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_dir_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all sectors:                      motion frames 60" in out.stdout
    assert "--ignore W,NW,SW:                 motion frames 60" in out.stdout
    assert "--ignore E,NE,SE,S, clock masked: motion frames 10" in out.stdout
