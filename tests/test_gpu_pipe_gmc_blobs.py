"""GPU tier (`-m gpu`): the compensated blob scan carried through the pipe (include/mtgpu_pipe_gmc_blobs.h;
csrc/gmc_blobs_kernels.hip, the pipe form), the C++ host layer and mtgpu_scan_file.  Expected values: numbers derived by
hand and the model (tests/pipe_gmc_blobs_inputs.py; both checked without a GPU by tests/test_pipe_gmc_blobs_host.py), and
for Q1 - Q4 mtgpu_scan_frames_gmc_blobs, the blob pipe and the compensated pipe on the same frames.  Every comparison is
exact."""
import contextlib
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import derived_cliff_inputs as dci
import gmc_blobs_inputs as gbi
import pipe_gmc_blobs_inputs as pq
import pipe_gmc_inputs as pg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
ZC, CE = m.LAYOUT_ZERO_COPY, m.LAYOUT_CENTRES
LAYOUTS = [rec | zc | CE for rec in (m.LAYOUT_COMPACT8, m.LAYOUT_AOS40) for zc in (0, ZC)]
LAYOUT_IDS = ["-".join([r] + z) for r in ("compact8", "aos40") for z in ([], ["zero-copy"])]
REPORTS = pq.REPORTS


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


def resident(s, frames, ms, q8, mb, keep=None):
    """mtgpu_scan_frames_gmc_blobs on the same frames — under `keep` as one stream that covers every frame — ->
    {report: (flags, counts)}."""
    frames = list(frames)
    args = () if keep is None else ([0, len(frames)], zones.pack_keep(np.asarray(keep, dtype=bool)))
    r = s.scan_gmc_blobs(m.FrameBatch.from_frames(frames), ms, q8, mb, *args)
    fl = r["flags"].tolist()
    vec = [pg.pack_vector(x, y) for x, y in zip(r["info"]["gx"].tolist(), r["info"]["gy"].tolist())]
    return {"centres": (fl, r["centres"].tolist()), "largest": (fl, r["largest"].tolist()), "vector": (fl, vec)}


def big_enough(frames):
    return 2 * max([len(f) for f in frames if f is not None] + [64])


# ------------------------------------------------------------------ 1. the rule bites

def test_the_rule_bites(gpu_scanner_factory):
    """P4 (four isolated pairs) and O8 (one object of eight cells) inside a pan of (9, 3), at min_blob_cells 3: set_gmc
    alone flags both (8 centres), set_blobs(3) alone flags both (one blob of 2360), the pair tells them apart.  P4 with a
    still overlay reads the overlay's 30 cells without a mask and P4's values under the mask that clears it.  Case D of
    pipe_gmc_inputs (the overlay in the majority) fails on a build that applies the mask only to the active plane."""
    p = pg.params()
    s = gpu_scanner_factory(p)
    fr = gbi.bite_frames()
    with contextlib.closing(m.ScanPipe(s, 16384, 2, 2, centres=True)) as pipe:
        assert pipe.gmc_blobs() is None
        both = [fr["P4"], fr["O8"]]
        pipe.set_gmc(pq.MS, pq.Q8, "centres")
        assert run(pipe, both) == ([pq.BITE_GMC_ALONE[0]] * 2, [pq.BITE_GMC_ALONE[1]] * 2)
        pipe.clear_gmc()
        for report, col in (("centres", 1), ("largest", 2)):
            pipe.set_blobs(3, report)
            assert run(pipe, both) == ([pq.BITE_BLOBS_ALONE[0]] * 2, [pq.BITE_BLOBS_ALONE[col]] * 2)
        pipe.set_blobs(0)
        for row in pq.BITE:
            name, frame, kp = row[:3]
            keep = gbi.BITE_KEEPS[kp]
            pipe.set_keep(keep)
            for report in REPORTS:
                pipe.set_gmc_blobs(pq.MIN_BLOB, pq.MS, pq.Q8, report)
                assert pipe.gmc_blobs() == (pq.MIN_BLOB, pq.MS, pq.Q8, report)
                assert run(pipe, [fr[frame]]) == ([row[3]], [pq.bite_count(row, report)]), (name, report)
        # the pair told apart in one batch
        pipe.set_keep(None)
        pipe.set_gmc_blobs(pq.MIN_BLOB, pq.MS, pq.Q8, "largest")
        assert run(pipe, both) == ([0, 1], [2, 8])
        # case D: without the keep bit in the estimate the mode stays 0 and the frame keeps 40 centres
        for keep in (None, pg.KEEP_D):
            pipe.set_keep(keep)
            for report in REPORTS:
                pipe.set_gmc_blobs(pq.MIN_BLOB, pq.MS, pq.Q8, report)
                want = pq.model(p, [fr["D"]], pq.MIN_BLOB, pq.MS, pq.Q8, report, keep)
                assert run(pipe, [fr["D"]]) == want, (keep is not None, report)
        assert want == ([0], [pg.pack_vector(9, 3)])


# ------------------------------------------------------------------ 2. Q1 - Q4 in every layout and batch shape

@pytest.fixture(scope="module")
def shapes_rows():
    """The model rows of shapes_case(), once: {(ms, q8, masked): rows}."""
    p, frames, keep = pg.shapes_case()
    return {(ms, q8, k): pq.rows(p, frames, ms, q8, keep if k else None) for ms, q8 in pg.SETTINGS for k in (False, True)}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_q1_to_q4_in_every_layout_and_batch_shape(gpu_scanner_factory, shapes_rows, layout):
    p, frames, keep = pg.shapes_case()
    s = gpu_scanner_factory(p)
    n = len(frames)
    ones = np.ones((pg.GH, pg.GW), dtype=bool)
    geoms = [(40000, 1, 2), (70000, 4, 2), (200000, n, 2), (4096, 5, 3)]       # one frame; 4; exactly the capacity; growing batches
    for gi, (max_rec, max_fr, nbuf) in enumerate(geoms):
        with contextlib.closing(m.ScanPipe(s, max_rec, max_fr, nbuf, layout=layout)) as pipe:
            plain = run(pipe, frames)
            for ms, q8 in (pg.SETTINGS if gi == 1 else pg.SETTINGS[:1] + pg.SETTINGS[2:3]):
                for mb in ((1, 3) if gi == 1 else (3,)):
                    for kp in (None, keep):
                        pipe.set_keep(kp)
                        rows = shapes_rows[(ms, q8, kp is not None)]
                        res = resident(s, frames, ms, q8, mb, kp)
                        for report in REPORTS:
                            want = pq.answers(p, rows, mb, report)
                            pipe.set_gmc_blobs(mb, ms, q8, report)
                            got = run(pipe, frames)
                            assert got == want, (max_fr, ms, q8, mb, kp is not None, report)          # the model
                            assert got == res[report], (max_fr, ms, q8, mb, kp is not None, report)   # Q1
                            if kp is None and gi == 1:                                             # Q2: all ones == none
                                pipe.set_keep(ones)
                                assert run(pipe, frames) == got, (ms, q8, mb, report)
                                pipe.set_keep(None)
                            if ms == 0:                                                            # Q3
                                if report == "vector":
                                    assert not any(got[1])
                                else:
                                    pipe.clear_gmc_blobs()
                                    pipe.set_blobs(mb, report)
                                    assert run(pipe, frames) == got, (mb, kp is not None, report)
                                    pipe.set_blobs(0)
                            if mb == 1 and report != "largest":                                    # Q4
                                pipe.clear_gmc_blobs()
                                pipe.set_gmc(ms, q8, report)
                                assert run(pipe, frames) == got, (ms, q8, kp is not None, report)
                                pipe.clear_gmc()
                        pipe.clear_gmc_blobs()
            pipe.set_keep(None)
            assert pipe.gmc_blobs() is None and run(pipe, frames) == plain        # off: the plain pipe again, bit for bit
    with contextlib.closing(m.ScanPipe(s, 40000, 1, 1, layout=layout)) as pipe:      # one frame through a pipe of one batch
        pipe.set_keep(keep)
        pipe.set_gmc_blobs(3, 16, 64, "vector")
        want = pq.answers(p, shapes_rows[(16, 64, True)], 3, "vector")
        for i in (1, 4, 0, 5):
            assert run(pipe, frames[i:i + 1]) == (want[0][i:i + 1], want[1][i:i + 1]), i


# ------------------------------------------------------------------ 3. both exits write

@pytest.mark.parametrize("layout", [m.LAYOUT_COMPACT8 | ZC, m.LAYOUT_AOS40 | ZC], ids=["compact8-zero-copy", "aos40-zero-copy"])
@pytest.mark.parametrize("report", REPORTS)
def test_both_exits_write_into_a_reused_pinned_block(gpu_scanner_factory, layout, report):
    """n_buffers = 1, zero-copy: batch 1 (the labelled exit) leaves flag 1 / 8 / 8 / (9, 3) in every slot of the pinned
    block; batch 2 (the early exit: no centre) and batch 3 (no side data: the planning kernel) go into the same slots and
    must read their own values: 0 flags, 0 counts, and under `vector` batch 2's own (4, -2) and then 0."""
    p, one, two, three, hand = pq.stale_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 16384, 3, 1, layout=layout, centres=True)) as pipe:
        pipe.set_gmc_blobs(pq.MIN_BLOB, pq.MS, pq.Q8, report)
        for frames, h in ((one, hand[0]), (two, hand[1]), (three, hand[2]), (one, hand[0]), (three, hand[2]), (one, hand[0]),
                          (two, hand[1])):
            assert run(pipe, frames) == (h["flags"], h[report])
        mixed = [one[0], two[0], None]
        assert run(pipe, mixed) == ([1, 0, 0], [hand[0][report][0], hand[1][report][0], 0])
        assert run(pipe, mixed[::-1]) == ([0, 0, 1], [0, hand[1][report][0], hand[0][report][0]])


# ------------------------------------------------------------------ 4. word seams, VECTORS_NEEDED 0

def test_word_seams_under_the_pan_and_a_mask(gpu_scanner_factory):
    """Blobs across columns 63 | 64 under the pan embedding: without a mask the hand values of
    pipe_blobs_inputs.seam_case, with column 63 cleared the model — in both record layouts."""
    p, plain, masked, keep, hand = pq.seam_case()
    s = gpu_scanner_factory(p)
    vec = [pg.pack_vector(*pq.SEAM_PAN)] * len(plain)
    for layout in (m.LAYOUT_COMPACT8 | ZC | CE, m.LAYOUT_AOS40 | CE):
        with contextlib.closing(m.ScanPipe(s, big_enough(plain + masked), 3, 2, layout=layout)) as pipe:
            for report, want in (("centres", hand["centres"]), ("largest", hand["largest"]), ("vector", vec)):
                pipe.set_gmc_blobs(5, pq.MS, pq.Q8, report)
                flags = [int(c >= 1 and g >= 5) for c, g in zip(hand["centres"], hand["largest"])]
                assert flags == [1, 1, 1, 0]
                assert run(pipe, plain) == (flags, want) == pq.model(p, plain, 5, pq.MS, pq.Q8, report), report
            pipe.set_keep(keep)
            for report in REPORTS:
                pipe.set_gmc_blobs(4, pq.MS, pq.Q8, report)
                assert run(pipe, masked) == pq.model(p, masked, 4, pq.MS, pq.Q8, report, keep), report
            pipe.clear_gmc_blobs()


def test_vectors_needed_zero_under_a_mask(gpu_scanner_factory):
    p, frames, keep = pq.vn0_case()
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, 4096, 2, 2, centres=True)) as pipe:
        for kp in (None, keep):
            pipe.set_keep(kp)
            for report in REPORTS:
                pipe.set_gmc_blobs(2, pq.MS, pq.Q8, report)
                got = run(pipe, frames)
                assert got == pq.model(p, frames, 2, pq.MS, pq.Q8, report, kp), (kp is not None, report)
                if kp is None and report != "vector":
                    assert got == ([1], [118 * 68])


# ------------------------------------------------------------------ 5. random batches

@pytest.mark.parametrize("i", gbi.RANDOM, ids=["%dx%d-mask%g-vn%d" % c for c in gbi.zi.RANDOM_CASES])
def test_random_batches_against_the_model(gpu_scanner_factory, i):
    p, frames, keep, has, plain, masked = pq.random_case(i)
    s = gpu_scanner_factory(p)
    layout = (m.LAYOUT_COMPACT8 if i % 2 else m.LAYOUT_AOS40) | (ZC if i % 4 < 2 else 0) | CE
    with contextlib.closing(m.ScanPipe(s, big_enough(frames), 5, 2, layout=layout)) as pipe:
        for kp, want in ((None, plain), (keep, masked)):
            pipe.set_keep(kp)
            for report in REPORTS:
                pipe.set_gmc_blobs(2, pq.MS, 64, report)
                assert run(pipe, frames) == pq.batch_answers(p, want, has, 2, report), (kp is not None, report)


# ------------------------------------------------------------------ 6. limits

@pytest.mark.parametrize("name", ["tall-3", "wide-1"])
def test_last_grid_the_preview_accepts_and_the_first_it_rejects(gpu_scanner_factory, name):
    gw, gh, kind = gbi.limit_shapes()[name]
    p, frames, has, want = pq.limit_frames(name)
    s = gpu_scanner_factory(p)
    with contextlib.closing(m.ScanPipe(s, big_enough(frames), 4, 2, centres=True)) as pipe:
        for report in REPORTS:
            pipe.set_gmc_blobs(2, pq.MS, pq.Q8, report)
            assert run(pipe, frames) == pq.batch_answers(p, want, has, 2, report), report
    # one row / one column more: no form
    gw2, gh2 = (gw, gh + 1) if kind == "tall" else (gw + 1, gh)
    p2 = dci.grid_params(gw2, gh2, **gbi.LIMIT_KW)
    assert gbi.preview_or_none(p2) is None
    s2 = gpu_scanner_factory(p2)
    few = [f for f in frames if f is not None][:3] + [None]
    with contextlib.closing(m.ScanPipe(s2, big_enough(frames), 4, 2, centres=True)) as pipe:
        before = run(pipe, few)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc_blobs(2)
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and f"{gw2}x{gh2}" in str(e.value)
        assert pipe.gmc_blobs() is None and m.load_library().mtgpu_pipe_gmc_blobs(pipe._pipe, None, None, None, None) == 0
        assert run(pipe, few) == before == (s2.check_frames(m.FrameBatch.from_frames(few)).tolist(), before[1])


def test_row_banded_grid_is_unsupported(gpu_scanner_factory):
    """960 x 540 cells: set_gmc_blobs is MT_ERR_UNSUPPORTED with the grid named, the setting stays off and the pipe goes
    on scanning plainly."""
    from mvtrim_amd import synth
    p = m.ScanParams.from_config(3840, 2160, **gbi.FINE_KW)
    s = gpu_scanner_factory(p)
    spec = synth.spec_4k_fine(seed=3)
    spec.events = [synth.Event(1, 3, 400, 200, 6, 4, 9, 1)]
    frames = [synth.gen_frame(spec, i) for i in range(3)]
    with contextlib.closing(m.ScanPipe(s, 518400 * 2, 2, 2)) as pipe:
        before = run(pipe, frames)[0]
        assert before == [0, 1, 1]
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc_blobs(3)
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
        assert pipe.gmc_blobs() is None
        assert run(pipe, frames)[0] == before


def test_4k_serpentine_one_workgroup_per_cu(gpu_scanner_factory):
    p, frames, (centres, largest, pan) = pq.uhd_case()
    s = gpu_scanner_factory(p)
    assert (centres, largest) == (14817, 14817) and len(frames) == 8
    with contextlib.closing(m.ScanPipe(s, 8 * big_enough(frames), 8, 2, centres=True)) as pipe:
        for report, count in (("centres", centres), ("largest", largest), ("vector", pg.pack_vector(*pan))):
            pipe.set_gmc_blobs(14817, pq.MS, pq.Q8, report)
            assert run(pipe, frames) == ([1] * 8, [count] * 8), report
        pipe.set_gmc_blobs(14818, pq.MS, pq.Q8, "largest")
        assert run(pipe, frames) == ([0] * 8, [largest] * 8)


# ------------------------------------------------------------------ 7. the state machine

def test_bad_arguments_change_nothing(gpu_scanner_factory):
    p = pg.params()
    s = gpu_scanner_factory(p)
    lib = m.load_library()
    fr = gbi.bite_frames()
    frames = [fr["P4"], fr["O8"]]
    with contextlib.closing(m.ScanPipe(s, 16384, 2, 2)) as pipe:                # no MT_LAYOUT_CENTRES
        bad = [((3, -1, 128, 0), "max_shift"), ((3, 128, 128, 0), "max_shift"), ((3, 16, -1, 0), "min_share_q8"),
               ((3, 16, 257, 0), "min_share_q8"), ((3, 16, 128, 3), "report"), ((3, 16, 128, -1), "report"),
               ((3, 16, 128, _abi.MT_PIPE_REPORT_LARGEST), "MT_LAYOUT_CENTRES"), ((3, 16, 128, _abi.MT_PIPE_REPORT_VECTOR), "MT_LAYOUT_CENTRES"),
               ((-1, 16, 128, 0), "min_blob_cells")]
        for state in (None, (8, 12, 200, "centres")):
            if state:
                pipe.set_gmc_blobs(*state)
            for args, word in bad:
                assert lib.mtgpu_pipe_set_gmc_blobs(pipe._pipe, *args) == _abi.MT_ERR_INVALID, args
                assert word in lib.mtgpu_last_error().decode(), args
                assert pipe.gmc_blobs() == state
        with pytest.raises(ValueError):
            pipe.set_gmc_blobs(3, 16, 128, "blobs")
        assert run(pipe, frames)[0] == [0, 1]                                   # min_blob_cells 8: P4's pairs fail, O8 passes
        assert lib.mtgpu_pipe_set_gmc_blobs(pipe._pipe, 0, 999, -5, 77) == _abi.MT_OK and pipe.gmc_blobs() is None   # ignored at 0
        a, b, c, d = ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_int32(7), ctypes.c_int(7)
        assert lib.mtgpu_pipe_gmc_blobs(pipe._pipe, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d)) == 0
        assert (a.value, b.value, c.value, d.value) == (7, 7, 7, 7)
        assert run(pipe, frames)[0] == [1, 1]
    with contextlib.closing(m.ScanPipe(s, 16384, 2, 2, centres=True)) as pipe:
        pipe.set_gmc_blobs(5, 7, 100, "vector")
        assert lib.mtgpu_pipe_gmc_blobs(pipe._pipe, None, None, None, None) == 1 and pipe.gmc_blobs() == (5, 7, 100, "vector")
        pipe.clear_gmc_blobs()
        pipe.set_gmc_blobs(2)                                                   # the other arguments were reset at 0
        assert pipe.gmc_blobs() == (2, 16, 128, "centres")


def test_conflicts_with_the_single_modes_in_both_orders(gpu_scanner_factory):
    p = pg.params()
    s = gpu_scanner_factory(p)
    fr = gbi.bite_frames()
    frames = [fr["P4"], fr["O8"], None, fr["P4+overlay"]]
    with contextlib.closing(m.ScanPipe(s, 16384, 4, 2, centres=True)) as pipe:
        # a single mode is on: the pair is refused, the mode that is on is named, nothing changes
        pipe.set_blobs(3, "largest")
        before = run(pipe, frames)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc_blobs(3)
        assert e.value.code == _abi.MT_ERR_INVALID and "mtgpu_pipe_set_blobs" in str(e.value) and "turn it off first" in str(e.value)
        assert pipe.gmc_blobs() is None and pipe.blobs == (3, "largest") and run(pipe, frames) == before
        pipe.set_blobs(0)
        pipe.set_gmc(16, 128, "vector")
        before = run(pipe, frames)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc_blobs(3)
        assert e.value.code == _abi.MT_ERR_INVALID and "mtgpu_pipe_set_gmc)" in str(e.value) and "turn it off first" in str(e.value)
        assert pipe.gmc_blobs() is None and pipe.gmc() == (16, 128, "vector") and run(pipe, frames) == before
        pipe.clear_gmc()
        # the pair is on: the two single setters are refused, this setter is named, nothing changes
        pipe.set_gmc_blobs(3, 16, 128, "largest")
        before = run(pipe, frames)
        assert before == pq.model(p, frames, 3, 16, 128, "largest")
        for call in (lambda: pipe.set_blobs(3, "largest"), lambda: pipe.set_gmc(16, 128, "centres")):
            with pytest.raises(m.MtgpuError) as e:
                call()
            assert e.value.code == _abi.MT_ERR_INVALID and "mtgpu_pipe_set_gmc_blobs" in str(e.value)
            assert pipe.gmc_blobs() == (3, 16, 128, "largest") and pipe.blobs is None and pipe.gmc() is None
            assert run(pipe, frames) == before
        # their off calls stay MT_OK and leave the pair alone
        pipe.set_blobs(0)
        pipe.clear_gmc()
        assert pipe.gmc_blobs() == (3, 16, 128, "largest") and run(pipe, frames) == before
        lib = m.load_library()
        assert lib.mtgpu_pipe_blobs(pipe._pipe, None, None) == 0 and lib.mtgpu_pipe_gmc(pipe._pipe, None, None, None) == 0
        # and the single modes still refuse each other as before
        pipe.clear_gmc_blobs()
        pipe.set_blobs(3)
        with pytest.raises(m.MtgpuError) as e:
            pipe.set_gmc()
        assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "not together yet" in str(e.value)


def test_busy_and_commuting_with_set_keep(gpu_scanner_factory):
    p = pg.params()
    s = gpu_scanner_factory(p)
    fr = gbi.bite_frames()
    frames = [fr["P4+overlay"], fr["O8"], None, fr["D"], fr["P4"]]
    keep = pg.KEEP_C
    a = pq.model(p, frames, 3, 16, 128, "largest")
    b = pq.model(p, frames, 3, 16, 128, "largest", keep)
    assert a != b
    with contextlib.closing(m.ScanPipe(s, 16384, 2, 3, centres=True)) as pipe:
        pipe.set_gmc_blobs(3, 16, 128, "largest")
        feed_all(pipe, frames[:1])                                              # a batch being filled
        for call in (lambda: pipe.set_gmc_blobs(5, 3, 0, "vector"), pipe.clear_gmc_blobs):
            with pytest.raises(m.MtgpuError) as e:
                call()
            assert e.value.code == _abi.MT_ERR_BUSY and "being filled" in str(e.value) and pipe.gmc_blobs() == (3, 16, 128, "largest")
        for i in range(1, len(frames)):
            pipe.feed(frames[i], float(i), tag=i)
        out = pipe.drain_centres()
        assert ([fl for _, fl, _, _ in out], [c for _, _, _, c in out]) == a
    results = []
    for order in ("keep-first", "pair-first"):
        with contextlib.closing(m.ScanPipe(s, 16384, 2, 2, centres=True)) as pipe:
            if order == "keep-first":
                pipe.set_keep(keep)
                pipe.set_gmc_blobs(3, 16, 128, "largest")
            else:
                pipe.set_gmc_blobs(3, 16, 128, "largest")
                pipe.set_keep(keep)
            assert pipe.has_keep and pipe.gmc_blobs() == (3, 16, 128, "largest")
            x = run(pipe, frames)
            pipe.set_keep(None)
            assert pipe.gmc_blobs() == (3, 16, 128, "largest")
            results.append((x, run(pipe, frames)))
    assert results[0] == results[1] == (b, a)


# ------------------------------------------------------------------ 8. no ring scratch, one event triple

def test_pair_submit_takes_no_ring_scratch_and_records_one_triple(gpu_scanner_factory):
    p, one, two, three, hand = pq.stale_case()
    s = gpu_scanner_factory(p)                                 # a context of its own: nothing else has launched on it
    high0 = s.stats()["pool_reserved_high"]
    with contextlib.closing(m.ScanPipe(s, 16384, 1, 2, centres=True)) as pipe:
        pipe.set_keep(pg.ONES)
        pipe.set_gmc_blobs(pq.MIN_BLOB, pq.MS, pq.Q8, "vector")
        s.profile(True)
        try:
            s.profile_read()
            assert run(pipe, one) == (hand[0]["flags"], hand[0]["vector"])      # three batches of one frame
            r = s.profile_read()
        finally:
            s.profile(False)
        assert r["launches"] == 3 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
        assert s.stats()["pool_reserved_high"] == high0


# ------------------------------------------------------------------ 9. mtgpu_scan_file, the host layer, the example

MERGE_ENV = dict(MAX_GAP_SEC="0.1", PADDING_SEC="0.04", MIN_SAVINGS_PCT="5", CHUNK_DURATION_SEC="1", TARGET_FPS="25")


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    """The 40-frame shaking recording with its overlay as a .mtmv file, the overlay's mask as a .mtkeep file."""
    d = tmp_path_factory.mktemp("pipe_gmc_blobs")
    p, frames, pts, keep = pg.recording_case()
    path = str(d / "shake.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, pg.REC_FPS, pg.REC_FRAMES / pg.REC_FPS, list(range(pg.REC_FRAMES)), list(frames))
    mask = str(d / "overlay.mtkeep")
    zones.save_keep(mask, keep)
    env = dict(os.environ, **MERGE_ENV)
    for k in ("CLUSTERS_NEEDED", "VECTORS_NEEDED", "MV_THRESHOLD_SQ", "BLOCK_SIZE", "BLOCK_SHIFT", "VERTICAL_MASK", "MTGPU_STAGING"):
        env.pop(k, None)
    return path, mask, env


@pytest.fixture(scope="module")
def recording_rows():
    """{(max_shift, masked): model rows} of the recording."""
    p, frames, _, keep = pg.recording_case()
    return {(ms, k): pq.rows(p, frames, ms, 128, keep if k else None) for ms in (16, 3) for k in (False, True)}


def python_segments(s, flags, pts):
    mp = m.MergeParams(duration=pg.REC_FRAMES / pg.REC_FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    seg, res = s.merge_segments(np.asarray(pts)[np.asarray(flags) != 0], mp, job_semantics=True)
    return [[float(a), float(b)] for a, b in seg.tolist()], res


def scan_file(env, path, *args):
    out = subprocess.run([os.path.join(PKG, "mtgpu_scan_file"), path, "--threads", "2"] + list(args), capture_output=True,
                         text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def test_scan_file_gmc_blobs_keep_and_sweep(gpu_scanner_factory, recording, recording_rows):
    """The recording's overlay is one residual blob of 30 cells in every frame with a non-zero pan; its object is 2 x 2
    cells in frames 10 .. 19.  --gmc-blobs 3 keeps the overlay's frames, --gmc-blobs 3 --keep only the object's, and
    --gmc-blobs 5 --keep nothing."""
    path, mask, env = recording
    p, frames, pts, keep = pg.recording_case()
    s = gpu_scanner_factory(p)
    plain = scan_file(env, path)
    assert "largest" not in plain and "sweep_gmc_blobs" not in plain
    kept = {}
    for keep_args, masked, levels in (([], False, [3, 30, 31]), (["--keep", mask], True, [2, 4, 5])):
        rows = recording_rows[(16, masked)]
        largest = pq.answers(p, rows, 1, "largest")[1]
        by_level = {}
        for n in levels:
            fl, ce = pq.answers(p, rows, n, "centres")
            want_seg, want_res = python_segments(s, fl, pts)
            r = scan_file(env, path, "--gmc-blobs", str(n), *keep_args)
            assert r["motion_frames"] == sum(fl) and r["segments"] == want_seg and r["do_cut"] == want_res["do_cut"], (n, masked)
            assert r["frames_scanned"] == pg.REC_FRAMES and ("ignored_cells" in r) == masked and "largest" not in r
            by_level[n] = r
            kept[(n, masked)] = r["motion_frames"]
        c = scan_file(env, path, "--gmc-blobs", str(levels[0]), "--centres", *keep_args)
        assert [n for _, n in c["centres"]] == pq.answers(p, rows, levels[0], "centres")[1]
        assert c["segments"] == by_level[levels[0]]["segments"]
        sw = scan_file(env, path, "--sweep-gmc-blobs", ",".join(map(str, levels)), *keep_args)
        # pts as the host layer computes them from a .mtmv with time base 1 / 25: frame->pts * av_q2d(time_base) (:361)
        assert sw["largest"] == [[float(f) * (1.0 / pg.REC_FPS), n] for f, n in enumerate(largest)]
        assert [e["min_blob_cells"] for e in sw["sweep_gmc_blobs"]] == levels and "sweep_blobs" not in sw
        assert sw["motion_frames"] == sum(pq.answers(p, rows, 1, "centres")[0])      # the sweep's own pass runs at 1 cell
        for e in sw["sweep_gmc_blobs"]:
            r = by_level[e["min_blob_cells"]]
            assert e["segments"] == r["segments"] and e["do_cut"] == r["do_cut"] and e["n_timestamps"] == r["n_timestamps"]
    # the model's counts: the overlay's 30 cells keep 25 of the 27 moving frames at 30 cells and none at 31; under the mask
    # the object's 4 cells keep its 10 frames up to 4 cells
    assert kept == {(3, False): 27, (30, False): 25, (31, False): 0, (2, True): 10, (4, True): 10, (5, True): 0}
    # the two parameters
    fl = pq.answers(p, recording_rows[(3, True)], 3, "centres")[0]
    r = scan_file(env, path, "--gmc-blobs", "3", "--gmc-blobs-max-shift", "3", "--keep", mask)
    assert r["motion_frames"] == sum(fl) != 10 and r["segments"] == python_segments(s, fl, pts)[0]
    fl = pq.model(p, frames, 3, 16, 256, "centres")[0]
    r = scan_file(env, path, "--gmc-blobs", "3", "--gmc-blobs-min-share-q8", "256")
    assert r["motion_frames"] == sum(fl) and r["segments"] == python_segments(s, fl, pts)[0]


def test_next_video_does_not_inherit_the_pair_setting(recording, recording_rows, tmp_path):
    """run_scan_pipeline on one pool of GpuBackends (tests/cpp/pipe_gmc_blobs_two_videos.cpp): the pair at 5 cells, plain,
    the pair at 31 cells and max_shift 3 (where the uncompensated pan rows are one blob of 472), and the pair together with min_blob_cells, refused before any decode."""
    path, _, env = recording
    p, frames, pts, _ = pg.recording_case()
    exe = str(tmp_path / "pipe_gmc_blobs_two_videos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "pipe_gmc_blobs_two_videos.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, path, "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    runs = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("run ")]
    assert len(runs) == 4
    want = [pq.answers(p, recording_rows[(16, False)], 5, "centres")[0], pg.masked_plain(p, frames)[0],
            pq.answers(p, recording_rows[(3, False)], 31, "centres")[0]]
    assert [sum(w) for w in want] == [25, 27, 24]
    for i, r in enumerate(runs[:3]):
        kv = dict(zip(r[0::2], r[1::2]))
        ts = [float(t) for t in kv["timestamps"].split(",") if t != "-"]
        assert ts == [pts[f] for f in range(pg.REC_FRAMES) if want[i][f]], i
        assert int(kv["motion_frames"]) == sum(want[i]) and int(kv["frames_scanned"]) == pg.REC_FRAMES
        assert kv["pair"].split(",") == [("5:16", "-", "31:3")[i]] * 2
    assert runs[3][:6] == ["run", "3", "rc", "1", "frames_scanned", "0"] and "min_blob_cells" in " ".join(runs[3])


def test_plain_c_pipe_gmc_blobs_example(tmp_path):
    exe = str(tmp_path / "pipe_gmc_blobs_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_gmc_blobs_example.c"), "-o", exe, "-L" + PKG, "-lmtgpu",
                           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plain scan:                          motion frames 290" in out.stdout
    assert "compensated (set_gmc):               motion frames 290" in out.stdout
    assert "blobs of 3 cells (set_blobs):        motion frames 290" in out.stdout
    assert "compensated blobs (set_gmc_blobs):   motion frames 29" in out.stdout
