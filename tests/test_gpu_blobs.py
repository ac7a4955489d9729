"""GPU tier (`-m gpu`): motion blobs — the connected components of a frame's centre cells (include/mtgpu_blobs.h,
csrc/blobs_kernels.hip).

Expected values: numbers written out by hand in tests/blobs_inputs.py; the numpy restatement tests/blobs_model.py (flood
fill) where a case says so; mtgpu_scan_centres_device / mtgpu_scan_zones_device (existing code) for `centres` and for
`flags` at min_blob_cells <= 1.  tests/test_blobs_host.py holds all of them against each other and against the oracle
without a GPU.  Every comparison is exact; outputs are pre-filled with junk: every element must be written by the call."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import blobs, tune

import blobs_inputs as bi
import blobs_model as bm
import zones_inputs as zi
from scan_checks import device_centres_of, to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK, JUNK_FLAG, JUNK_BOX = -7, 9, 0x1234
OUTPUTS = ("flags", "centres", "blobs", "largest", "box")
COUNTS = ("centres", "blobs", "largest")


# ------------------------------------------------------------------ device helpers

def soff_tensor(stream_off):
    import torch
    return torch.from_numpy(np.asarray(stream_off).astype(np.int64)).cuda()


def keep_tensor(keeps):
    import torch
    return torch.from_numpy(zi.pack_keeps(keeps).view(np.int64).copy()).cuda()


def junk_outputs(n, want=OUTPUTS):
    import torch
    out = {}
    for k in want:
        if k == "flags":
            out[k] = torch.full((n,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
        elif k == "box":
            out[k] = torch.full((n, 4), JUNK_BOX, dtype=torch.int16, device="cuda")
        else:
            out[k] = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    return out


def to_host(res):
    out = {}
    for k, t in res.items():
        if t is not None:
            a = t.cpu().numpy()
            out[k] = a if k == "flags" else a.view(np.uint16) if k == "box" else a.view(np.uint32)
    return out


def device_blobs(s, d_rec, d_off, d_sd, compact, min_blob=1, d_soff=None, d_keep=None, want=OUTPUTS, stream=None):
    """Through mtgpu_scan_blobs_device into junk-filled outputs -> {name: numpy array} on the host."""
    import torch
    out = junk_outputs(d_off.numel() - 1, want)
    torch.cuda.synchronize()
    res = s.scan_blobs_device(d_rec, d_off, d_sd, min_blob, d_soff, d_keep, compact=compact, want=want, out=out, stream=stream)
    torch.cuda.synchronize()
    return to_host(res)


def both_layouts(s, c, what, masked=False, min_blob=1):
    """Both record layouts through the device entry point; yields (label, outputs)."""
    d_soff = soff_tensor(c.soff) if masked else None
    d_keep = keep_tensor(c.keeps) if masked else None
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, compact)
        yield f"{what}, {'compact' if compact else '40-byte'}", device_blobs(s, d_rec, d_off, d_sd, compact, min_blob, d_soff, d_keep)


def assert_outputs(got, want, what, p=None, min_blob=1):
    """got: the call's outputs; want: {"centres", "blobs", "largest": per frame, "box": [F] of 4} — hand lists or the
    model's arrays.  Exact; flags, where p is given, from include/mtgpu_blobs.h's rule on the expected counts."""
    for k in COUNTS:
        g, w = got[k].astype(np.int64), np.asarray(want[k]).astype(np.int64)
        bad = np.flatnonzero(g != w)
        assert g.shape == w.shape and bad.size == 0, (f"{what}: {k} of {bad.size} of {w.size} frames differ, first {bad[:8].tolist()}: "
                                                      f"want {w[bad[:8]].tolist()} got {g[bad[:8]].tolist()}")
    gb, wb = got["box"].astype(np.int64).reshape(-1, 4), np.asarray(want["box"]).astype(np.int64).reshape(-1, 4)
    bad = np.flatnonzero((gb != wb).any(axis=1))
    assert bad.size == 0, f"{what}: boxes of frames {bad[:8].tolist()} differ: want {wb[bad[:8]].tolist()} got {gb[bad[:8]].tolist()}"
    if p is not None:
        wf = bm.flags_np(p, want["centres"], want["largest"], min_blob)
        assert got["flags"].tolist() == wf.tolist(), (what, "flags", got["flags"].tolist(), wf.tolist())


def assert_identities(got, what):
    c, b, g = (got[k].astype(np.int64) for k in COUNTS)
    assert ((b == 0) == (c == 0)).all() and ((g == 0) == (c == 0)).all(), what
    assert (g <= c).all() and (b * g >= c).all(), what
    none = (got["box"].reshape(-1, 4) == 0xFFFF).all(axis=1)
    assert (none == (b == 0)).all(), what


def run_hand_case(s, c, what, masked=False, hand=None):
    hand = c.hand if hand is None else hand
    for label, got in both_layouts(s, c, what, masked):
        assert_outputs(got, hand, label, c.p)
        assert_identities(got, label)


# ------------------------------------------------------------------ 1. centre cells only

def test_edge_columns_join_nothing(gpu_scanner_factory):
    """Two centres that touch only through a cell of column 0 (then column gw - 1), which is no centre: two blobs."""
    c = bi.edge_columns_case()
    run_hand_case(gpu_scanner_factory(c.p), c, "edge columns")


def test_halo_rows_join_nothing(gpu_scanner_factory):
    """Margin 1, vn == 0, keep masks: two centres that touch only through halo-row cells are two blobs; a pair on the last
    analysed row is one; the edge columns again."""
    c = bi.halo_row_case()
    run_hand_case(gpu_scanner_factory(c.p), c, "halo row", masked=True)


# ------------------------------------------------------------------ 2. word seams

@pytest.mark.parametrize("gw", bi.SEAM_GW)
def test_word_seams(gpu_scanner_factory, gw):
    """A bar across the 64-cell seams is one blob; with one cell next to a seam cleared by the stream's mask it falls
    apart as derived by hand; with keep NULL it is one again."""
    c = bi.seam_case(gw)
    s = gpu_scanner_factory(c.p)
    run_hand_case(s, c, f"seam gw {gw}, masks", masked=True)
    one = {k: [v[0]] * len(v) for k, v in c.hand.items()}
    run_hand_case(s, c, f"seam gw {gw}, no mask", hand=one)


# ------------------------------------------------------------------ 3. late merges

def test_late_merges(gpu_scanner_factory):
    """A comb joined only on the last analysed row, a U, a ring with a separate blob inside (20 x 12, by hand)."""
    c = bi.late_merge_case()
    run_hand_case(gpu_scanner_factory(c.p), c, "comb / U / ring")


# ------------------------------------------------------------------ 4. thin and long

@pytest.mark.parametrize("which", ["66x12", "4k", "spiral"])
def test_thin_and_long(gpu_scanner_factory, which):
    """One path of 389 (66 x 12), 14 817 (4K grid, eight frames in one batch) and 3 719 cells (a square spiral on the
    1080p grid): blobs 1, largest = the path length.  Legitimate inputs: they converge, nothing retries."""
    c = bi.serpentine_case(which)
    if which == "spiral":
        assert c.hand["largest"] == [3719]
    run_hand_case(gpu_scanner_factory(c.p), c, f"thin path {which}")


# ------------------------------------------------------------------ 5. many blobs

@pytest.mark.parametrize("which", ["1080p", "4k"])
def test_many_blobs(gpu_scanner_factory, which):
    """Dominoes in a brick pattern: more blobs than any bounded label table holds.  Expected: the model (which the host
    tier holds to the construction's own count)."""
    c = bi.domino_case(which)
    want = bm.model_batch(c.p, c.mv, c.off, c.sd)
    assert int(want["blobs"][0]) == c.hand["blobs"][0] > 1024 and int(want["largest"][0]) == 2
    s = gpu_scanner_factory(c.p)
    for label, got in both_layouts(s, c, f"dominoes {which}"):
        assert_outputs(got, want, label, c.p)


# ------------------------------------------------------------------ 6. one blob of everything

@pytest.mark.parametrize("margin", [6, 0])
def test_one_blob_of_everything(gpu_scanner_factory, margin):
    """vn == 0, side data, no record, no mask, 240 x 135: every analysed cell of columns 1 .. 238 in one blob."""
    c = bi.everything_case(margin)
    if margin == 6:
        assert c.hand == {"centres": [29274], "blobs": [1], "largest": [29274], "box": [(1, 6, 238, 128)]}
    run_hand_case(gpu_scanner_factory(c.p), c, f"everything, margin {margin}")


# ------------------------------------------------------------------ 7. tie and box

def test_tie_and_box(gpu_scanner_factory):
    """Two blobs of three cells: the box is that of the one holding the smaller cell index, although the other lies
    further left; grown by one cell, the other one wins and the box moves."""
    c = bi.tie_case()
    s = gpu_scanner_factory(c.p)
    run_hand_case(s, c, "tie")
    # flags at min_blob_cells 3 and 4 (clusters_needed 1): frame 0's largest is 3
    for mb, want in ((3, [1, 1, 1]), (4, [0, 1, 1]), (5, [0, 0, 0])):
        for label, got in both_layouts(s, c, f"tie min_blob {mb}", min_blob=mb):
            assert got["flags"].tolist() == want, label


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    """With mtgpu_profile_enable on, one resident blob scan is one event triple, and its answers are the hand values."""
    c = bi.tie_case()
    s = gpu_scanner_factory(c.p)
    d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_blobs(s, d_rec, d_off, d_sd, False)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert got["centres"].tolist() == c.hand["centres"]
    assert_outputs(got, c.hand, "profiled call", c.p)


# ------------------------------------------------------------------ 8. batch plumbing

def test_batch_plumbing(gpu_scanner_factory):
    """Frames without side data, has_sd == 0 frames that own records, frames behind the last stream, an empty stream, a
    stream with an all-zero mask; n_frames == 0; every single-output call; a non-default stream."""
    import torch
    c = bi.plumbing_case()
    s = gpu_scanner_factory(c.p)
    run_hand_case(s, c, "plumbing, no mask", hand=c.hand["plain"])
    run_hand_case(s, c, "plumbing, masks", masked=True, hand=c.hand["masked"])
    d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, False)
    d_soff, d_keep = soff_tensor(c.soff), keep_tensor(c.keeps)
    # has_sd == NULL: side data iff records — frame 2 counts, frame 3 still has none
    plain = dict(c.hand["plain"])
    sd_null = {k: list(v) for k, v in plain.items()}
    for k, v in zip(OUTPUTS[1:], (35, 2, 32, (4, 2, 13, 9))):
        sd_null[k][2] = v
    assert_outputs(device_blobs(s, d_rec, d_off, None, False), sd_null, "has_sd NULL", c.p)
    # every single-output call: the four others NULL
    full = device_blobs(s, d_rec, d_off, d_sd, False, 4, d_soff, d_keep)
    lib = m.load_library()
    for i, name in enumerate(OUTPUTS):
        one = device_blobs(s, d_rec, d_off, d_sd, False, 4, d_soff, d_keep, want=(name,))
        assert list(one) == [name] and np.array_equal(one[name], full[name]), name
        # the raw call: five junk-filled tensors exist, one is handed in — the other four keep their junk
        junk = junk_outputs(len(c.sd))
        ptrs = [junk[k].data_ptr() if k == name else None for k in OUTPUTS]
        torch.cuda.synchronize()
        rc = lib.mtgpu_scan_blobs_device(s._ctx, d_rec.data_ptr(), 40, len(c.mv), d_off.data_ptr(), d_sd.data_ptr(), len(c.sd),
                                         d_soff.data_ptr(), len(c.soff) - 1, d_keep.data_ptr(), 4, *ptrs, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.mtgpu_last_error()
        got = to_host(junk)
        assert np.array_equal(got[name], full[name]), name
        fresh = to_host(junk_outputs(len(c.sd)))
        for other in OUTPUTS:
            if other != name:
                assert np.array_equal(got[other], fresh[other]), (name, "touched", other)
    assert full["flags"].tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 0]
    # a non-default stream
    st = torch.cuda.Stream()
    got = device_blobs(s, d_rec, d_off, d_sd, False, 1, d_soff, d_keep, stream=st.cuda_stream)
    st.synchronize()
    assert_outputs(got, c.hand["masked"], "non-default stream", c.p)
    # n_frames == 0: MT_OK, nothing written, through both entry points
    empty = to_device(c.mv[:0], c.off[:1], c.sd[:0], False)
    assert all(v.size == 0 for v in device_blobs(s, *empty, False).values())
    one = junk_outputs(1)
    rc = m.load_library().mtgpu_scan_blobs_device(s._ctx, None, 40, 0, d_off.data_ptr(), None, 0, None, 0, None, 1,
                                                  *(one[k].data_ptr() for k in OUTPUTS), None)
    torch.cuda.synchronize()
    assert rc == 0 and one["flags"].item() == JUNK_FLAG and one["centres"].item() == JUNK and one["box"][0, 0].item() == JUNK_BOX
    r = s.scan_blobs(m.FrameBatch(c.mv[:0], c.off[:1], None, c.sd[:0]))
    assert all(len(v) == 0 for v in r.values())
    # the host entry point, with and without masks, and a window that does not start at record 0
    r = s.scan_blobs(m.FrameBatch(c.mv, c.off, None, c.sd), 1)
    r["box"] = r["box"].view(np.uint16).reshape(-1, 4)
    assert_outputs(r, c.hand["plain"], "host entry", c.p)
    F = int(c.soff[-1])
    r = s.scan_blobs(m.FrameBatch(c.mv, c.off[:F + 1], None, c.sd[:F]), 1, c.soff, zi.pack_keeps(c.keeps))
    r["box"] = r["box"].view(np.uint16).reshape(-1, 4)
    assert_outputs(r, {k: v[:F] for k, v in c.hand["masked"].items()}, "host entry, masks", c.p)
    r = s.scan_blobs(m.FrameBatch(c.mv, c.off[4:8], None, c.sd[4:7]), 1)
    r["box"] = r["box"].view(np.uint16).reshape(-1, 4)
    assert_outputs(r, {k: v[4:7] for k, v in c.hand["plain"].items()}, "host entry, a window", c.p)
    with pytest.raises(ValueError):
        s.scan_blobs(m.FrameBatch(c.mv, c.off, None, c.sd), 1, c.soff, None)


# ------------------------------------------------------------------ 9. identities on random input

@pytest.mark.parametrize("i", range(len(zi.RANDOM_CASES)), ids=["%dx%d-mask%g-vn%d" % c for c in zi.RANDOM_CASES])
def test_random_input_identities(gpu_scanner_factory, i):
    """centres == mtgpu_scan_centres_device (mtgpu_scan_zones_device with masks); blobs, largest and box == the model;
    the three inequalities; flags at min_blob_cells 0 and 1 == the scan's flags, at 2, 3 and 5 == the model."""
    p, mv, off, sd, soff, keeps = zi.random_case(i)
    s = gpu_scanner_factory(p)
    for masked in (False, True):
        want = bm.model_batch(p, mv, off, sd, soff if masked else None, keeps if masked else None)
        d_soff, d_keep = (soff_tensor(soff), keep_tensor(keeps)) if masked else (None, None)
        for compact in (False, True):
            d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
            label = f"random {i}, {'masks' if masked else 'no mask'}, {'compact' if compact else '40-byte'}"
            if masked:
                fl, ce, _ = s.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, compact=compact)
                scan_f, scan_c = fl.cpu().numpy(), ce.cpu().numpy().view(np.uint32)
            else:
                scan_f, scan_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
            for mb in (0, 1, 2, 3, 5):
                got = device_blobs(s, d_rec, d_off, d_sd, compact, mb, d_soff, d_keep)
                assert got["centres"].tolist() == scan_c.tolist(), label
                assert_outputs(got, want, f"{label}, min_blob {mb}", p, mb)
                assert_identities(got, label)
                if mb <= 1:
                    assert got["flags"].tolist() == scan_f.tolist(), label
        assert int(want["blobs"].max()) >= 2


# ------------------------------------------------------------------ 10. sweep equivalence

def test_largest_through_the_sweep_is_flags_through_the_merge(gpu_scanner_factory):
    """clusters_needed 1, levels 1, 2, 4, 8: mtgpu_sweep_streams_device on `largest` == mtgpu_merge_streams_device on flags
    at min_blob_cells = L, segment for segment, bit patterns compared.  The input keeps all 96 frames at CLUSTERS_NEEDED
    8 and a quarter of them at MIN_BLOB_CELLS 8."""
    import torch
    p, mv, off, sd, pts, soff = bi.sweep_case()
    s = gpu_scanner_factory(p)
    CAP = 16
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_pts, d_soff = torch.from_numpy(pts.copy()).cuda(), soff_tensor(soff)
    mps = [m.MergeParams(duration=48 / 25.0, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0) for _ in range(2)]
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    levels = list(bi.SWEEP_LEVELS)
    res = s.scan_blobs_device(d_rec, d_off, d_sd, 1, compact=True)
    sseg, sres = s.sweep_streams_device(res["largest"], d_pts, d_soff, d_mp, levels, seg_cap=CAP)
    torch.cuda.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)        # noqa: E731
    kept, segs = [], []
    for li, lv in enumerate(levels):
        fl = s.scan_blobs_device(d_rec, d_off, d_sd, lv, compact=True, want=("flags",))["flags"]
        seg, r8 = s.merge_streams_device(fl, d_pts, d_soff, d_mp, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg.cpu().numpy())), lv
        assert np.array_equal(sres[li].cpu().numpy(), r8.cpu().numpy()), lv
        kept.append(int(fl.sum()))
        segs.append([int(r["n_segments"]) for r in m.results_from_bytes(r8.cpu().numpy())])
    assert kept == [96, 96, 48, 24] and segs[0] == [1, 1] and segs[3][0] >= 2


# ------------------------------------------------------------------ 11. the LDS limit

@pytest.mark.parametrize("kind", ["tall", "wide"])
def test_last_grid_the_preview_accepts(gpu_scanner_factory, kind):
    """The tallest 65-column grid and the widest 3-row grid that fit 160 KB: a serpentine over the whole grid, random
    blobs, pairs across the first and last seam on the first and last row — against the model."""
    c = bi.limit_case(kind)
    gw, gh = bi.limit_shapes()[kind]
    assert m.blobs_preview(c.p)["lds_bytes"] == bi.lds_by_hand(gw, gh) <= bi.MI355X_LDS
    want = bm.model_batch(c.p, c.mv, c.off, c.sd)
    assert want["blobs"].tolist()[0] == 1 and int(want["largest"][0]) == int(want["centres"][0]) > gw and int(want["blobs"][1]) > 4
    s = gpu_scanner_factory(c.p)
    for label, got in both_layouts(s, c, f"limit {kind} {gw}x{gh}"):
        assert_outputs(got, want, label, c.p)


# ------------------------------------------------------------------ 12. example and command

def test_plain_c_blobs_example(tmp_path):
    """examples/blobs_example.c: rain against one object, from plain C (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "blobs_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "blobs_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame 15: 16 centres in 5 blobs, largest 8 at (55, 30) .. (58, 31)" in out.stdout
    assert "motion frames: 60 of 60 with CLUSTERS_NEEDED 8, 10 with MIN_BLOB_CELLS 8" in out.stdout


def test_end_to_end_command(gpu_scanner_factory, tmp_path, capsys):
    """A .mtmv of the sweep input's first stream, then `python -m mvtrim_amd.blobs --json` in a fresh child process and
    the table form in this one: per level the object-size rule against the cell-count rule, and the histogram."""
    p, mv, off, sd, pts, soff = bi.sweep_case()
    F = 48
    frames = [mv[int(off[f]):int(off[f + 1])] for f in range(F)]
    path = str(tmp_path / "stream.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    batch, fpts, hdr = tune.load(path)
    assert batch.n_frames == F and hdr["width"] == 1920
    s = gpu_scanner_factory(p)
    mp = m.MergeParams(duration=F / 25.0, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    direct = blobs.measure(s, batch, fpts, [1, 2, 4, 8], mp)
    assert [r["min_blob_cells"]["motion_frames"] for r in direct["levels"]] == [48, 48, 24, 12]
    assert [r["clusters_needed"]["motion_frames"] for r in direct["levels"]] == [48, 48, 48, 48]
    assert direct["blobs_per_frame"]["4"] == 12 and direct["blobs_per_frame"]["5"] == 36 and direct["largest_blob"] == 9
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [path, "--vectors-needed", "1", "--max-gap-sec", "0.1", "--padding-sec", "0.04", "--min-savings-pct", "5"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.blobs"] + args + ["--json"], capture_output=True, text=True, env=env,
                         cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert doc["levels"] == direct["levels"] and doc["blobs_per_frame"] == direct["blobs_per_frame"]
    assert doc["levels"][3]["min_blob_cells"]["segments"] > doc["levels"][3]["clusters_needed"]["segments"] == 1
    # a keep mask that ignores the object's row 30: nothing larger than a pair is left
    from mvtrim_amd import zones
    keep = np.ones((68, 120), dtype=bool)
    keep[30] = False
    zones.save_keep(str(tmp_path / "row30.mtkeep"), keep)
    capsys.readouterr()
    assert blobs.main(args + ["--keep", str(tmp_path / "row30.mtkeep"), "--min-blob-cells", "2,3"]) == 0
    text = capsys.readouterr().out
    assert "the largest blob has 2 cells" in text and "blobs per frame:" in text and "MIN_BLOB_CELLS" in text
