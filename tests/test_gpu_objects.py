"""GPU tier (`-m gpu`): object lists — the K largest blobs of every frame, ranked and boxed (include/mtgpu_objects.h,
csrc/objects_kernels.hip, csrc/blob_rank.h).

Expected values: lists written out by hand in tests/objects_inputs.py; the numpy restatement tests/objects_model.py
(blobs_model's flood fill, then a sort) where a case says so; mtgpu_scan_blobs_device (existing code) on the same device
buffers for entry 0, centres, blobs and flags.  tests/test_objects_host.py holds the model and the hand values against
each other without a GPU.  Every comparison is exact; outputs are pre-filled with junk: every element must be written by
the call.  The cases run from the smallest grid to the largest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, objects, tune

import blob_planes as bp
import blobs_inputs as bi
import objects_inputs as oi
import objects_model as om
import test_gpu_blobs as tb
import zones_inputs as zi
from scan_checks import to_device

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("flags", "centres", "blobs", "objects", "list")
COUNTS = ("centres", "blobs", "objects")
JUNK, JUNK_FLAG = -7, 9


# ------------------------------------------------------------------ device helpers

def junk_outputs(n, k, want=OUTPUTS):
    import torch
    out = {}
    for name in want:
        if name == "flags":
            out[name] = torch.full((n,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
        elif name == "list":
            out[name] = torch.full((n, k, 4), JUNK, dtype=torch.int32, device="cuda")
        else:
            out[name] = torch.full((n,), JUNK, dtype=torch.int32, device="cuda")
    return out


def to_host(res):
    out = {}
    for name, t in res.items():
        if t is not None:
            a = t.cpu().numpy()
            out[name] = a if name == "flags" else a.view(om.OBJECT_DTYPE)[..., 0] if name == "list" else a.view(np.uint32)
    return out


def device_objects(s, d_rec, d_off, d_sd, compact, k=om.K_MAX, min_blob=1, min_objects=1, d_soff=None, d_keep=None, want=OUTPUTS,
                   stream=None):
    """Through mtgpu_scan_objects_device into junk-filled outputs -> {name: numpy array} on the host."""
    import torch
    out = junk_outputs(d_off.numel() - 1, k, want)
    torch.cuda.synchronize()
    res = objects.scan_device(s, d_rec, d_off, d_sd, k, min_blob, min_objects, d_soff, d_keep, compact=compact, want=want, out=out,
                              stream=stream)
    torch.cuda.synchronize()
    return to_host(res)


def layout_name(compact):
    return "compact" if compact else "40-byte"


def assert_outputs(got, want, what, p=None, min_objects=1):
    """got: the call's outputs; want: objects_model.model_batch's dict (or objects_inputs.hand_want's).  Exact."""
    for name in COUNTS:
        g, w = got[name].astype(np.int64), np.asarray(want[name]).astype(np.int64)
        bad = np.flatnonzero(g != w)
        assert g.shape == w.shape and bad.size == 0, (f"{what}: {name} of {bad.size} of {w.size} frames differ, first {bad[:8].tolist()}: "
                                                      f"want {w[bad[:8]].tolist()} got {g[bad[:8]].tolist()}")
    assert got["list"].shape == want["list"].shape, (what, got["list"].shape, want["list"].shape)
    bad = np.flatnonzero((got["list"] != want["list"]).any(axis=1))
    assert bad.size == 0, (f"{what}: lists of frames {bad[:4].tolist()} differ: want {want['list'][bad[:2]].tolist()} "
                           f"got {got['list'][bad[:2]].tolist()}")
    if p is not None:
        wf = om.flags_np(p, want["centres"], want["objects"], min_objects)
        assert got["flags"].tolist() == wf.tolist(), (what, "flags", got["flags"].tolist(), wf.tolist())


def assert_identities(got, what, min_blob):
    """Consequence D, the order of the list and its empties."""
    lst = got["list"]
    k = lst.shape[1]
    cells = lst["cells"].astype(np.int64)
    c, b, o = (got[n].astype(np.int64) for n in COUNTS)
    total = cells.sum(axis=1)
    assert (total <= c).all() and (total[b <= k] == c[b <= k]).all() and (o <= b).all(), what
    listed = (cells >= max(1, min_blob)).sum(axis=1)
    assert (o[listed < k] == listed[listed < k]).all() and (o >= listed).all(), what
    assert ((cells > 0).sum(axis=1) == np.minimum(b, k)).all(), what
    empty = cells == 0
    for name, none in (("first", 0xFFFFFFFF), ("x0", 0xFFFF), ("y0", 0xFFFF), ("x1", 0xFFFF), ("y1", 0xFFFF)):
        assert (lst[name][empty] == none).all(), (what, name)
    key = cells * (1 << 32) + (0xFFFFFFFF - lst["first"].astype(np.int64))           # empties: key 0, behind every blob
    assert (np.diff(key, axis=1)[~empty[:, 1:]] < 0).all() and (np.diff(empty.astype(np.int8), axis=1) >= 0).all(), what


def blob_scan(s, d_rec, d_off, d_sd, compact, min_blob, d_soff, d_keep):
    import torch
    out = tb.junk_outputs(d_off.numel() - 1)
    res = s.scan_blobs_device(d_rec, d_off, d_sd, min_blob, d_soff, d_keep, compact=compact, want=tb.OUTPUTS, out=out)
    torch.cuda.synchronize()
    return tb.to_host(res)


def assert_consequence_a(got, blob, what):
    """Entry 0 is the blob scan's largest and box; centres and blobs are the blob scan's."""
    lst = got["list"]
    assert got["centres"].tolist() == blob["centres"].tolist() and got["blobs"].tolist() == blob["blobs"].tolist(), what
    assert lst["cells"][:, 0].tolist() == blob["largest"].tolist(), what
    box = np.stack([lst[n][:, 0] for n in ("x0", "y0", "x1", "y1")], axis=1)
    assert np.array_equal(box, blob["box"].reshape(-1, 4)), what


# ------------------------------------------------------------------ 1. three blobs on the smallest grid

@pytest.mark.parametrize("masked", [False, True], ids=["no mask", "masks"])
def test_three_blobs_at_every_k(gpu_scanner_factory, masked):
    """63 x 12, by hand: blobs of 3, 3 and 2 cells at k = 1, 2, 3 and 16 — the tie goes to the smaller first, ranks beyond
    `blobs` read empty, the list for k is the head of the list for 16 (C); a frame without side data and one with side
    data and no record read zeros and an empty list; under the mask so does the frame behind the last stream."""
    c = oi.hand_case()
    s = gpu_scanner_factory(c.p)
    hand = c.hand["masked" if masked else "plain"]
    d_soff, d_keep = (tb.soff_tensor(c.soff), tb.keep_tensor(c.keeps)) if masked else (None, None)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, compact)
        full = device_objects(s, d_rec, d_off, d_sd, compact, 16, 1, 1, d_soff, d_keep)
        for k in (1, 2, 3, 16):
            for mbc, mo in ((1, 1), (3, 2), (3, 3), (4, 1), (0, 0)):
                what = f"three blobs, {layout_name(compact)}, k {k}, min_blob_cells {mbc}, min_objects {mo}"
                got = device_objects(s, d_rec, d_off, d_sd, compact, k, mbc, mo, d_soff, d_keep)
                assert_outputs(got, oi.hand_want(hand, k, mbc), what, c.p, mo)
                assert_identities(got, what, mbc)
                assert np.array_equal(got["list"], full["list"][:, :k]), what                    # C
        # every single-output call: the four others are not asked for
        for name in OUTPUTS:
            one = device_objects(s, d_rec, d_off, d_sd, compact, 3, 3, 2, d_soff, d_keep, want=(name,))
            ref = device_objects(s, d_rec, d_off, d_sd, compact, 3, 3, 2, d_soff, d_keep)
            assert list(one) == [name] and np.array_equal(one[name], ref[name]), name
    # the host entry point (its stream table ends at the batch's last frame: the first three frames under the mask)
    F = 3 if masked else 4
    r = objects.scan(s, m.FrameBatch(c.mv, c.off[:F + 1], None, c.sd[:F]), 3, 3, 2, *((c.soff, zi.pack_keeps(c.keeps)) if masked else ()))
    assert_outputs(r, oi.hand_want(hand[:F], 3, 3), "host entry", c.p, 2)
    assert r["list"].dtype == objects.OBJECT_DTYPE and r["list"].shape == (F, 3)
    with pytest.raises(ValueError):
        objects.scan(s, m.FrameBatch(c.mv, c.off, None, c.sd), 3, 1, 1, c.soff, None)


def test_profiled_call_records_one_triple(gpu_scanner_factory):
    """With mtgpu_profile_enable on, one object scan is one event triple, and its answers are the hand values."""
    c = oi.hand_case()
    s = gpu_scanner_factory(c.p)
    d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, False)
    s.profile(True)
    try:
        s.profile_read()
        got = device_objects(s, d_rec, d_off, d_sd, False, 4)
        r = s.profile_read()
    finally:
        s.profile(False)
    assert r["launches"] == 1 and r["scan_ms"] > 0.0 and r["plan_ms"] > 0.0
    assert_outputs(got, oi.hand_want(c.hand["plain"], 4), "profiled call", c.p)


# ------------------------------------------------------------------ 2. the centre planes of blob_planes

@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_centre_planes_against_the_model(gpu_scanner_factory, name):
    """Percolation, mazes, combs, bars and confetti at k = 16, 40-byte and compact records: all five outputs are the
    model's; on the same device buffers, entry 0 / centres / blobs are mtgpu_scan_blobs_device's (A) and the flags at
    min_objects 1 are its flags at the same min_blob_cells (B), masked batches included."""
    b, want = bp.batch(name), oi.expected(name)
    s = gpu_scanner_factory(b.p)
    d_soff, d_keep = (None, None) if b.keeps is None else (tb.soff_tensor(b.soff), tb.keep_tensor(b.keeps))
    mid = max(2, int(np.median(want["list"]["cells"][:, 0])))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(b.mv, b.off, b.sd, compact)
        what = f"{name}, {layout_name(compact)}"
        got = device_objects(s, d_rec, d_off, d_sd, compact, 16, 1, 1, d_soff, d_keep)
        assert_outputs(got, want, what, b.p, 1)
        assert_identities(got, what, 1)
        for mbc in (1, mid):
            blob = blob_scan(s, d_rec, d_off, d_sd, compact, mbc, d_soff, d_keep)
            mine = got if mbc == 1 else device_objects(s, d_rec, d_off, d_sd, compact, 16, mbc, 1, d_soff, d_keep)
            assert_consequence_a(mine, blob, what)
            assert mine["flags"].tolist() == blob["flags"].tolist(), (what, "B", mbc)
            assert np.array_equal(mine["list"], got["list"]), (what, "F", mbc)
            assert_identities(mine, what, mbc)
    if "confetti" in b.names:                       # every listed blob has 3 cells: the order is the tie rule alone
        f = b.frame_of["confetti"]
        assert set(got["list"]["cells"][f].tolist()) == {3} and int(got["blobs"][f]) > 16


# ------------------------------------------------------------------ 3. more candidates in one word than k

def test_more_blobs_in_one_word_than_k(gpu_scanner_factory):
    """21 pairs in word 0 of one row of 120 x 68: at k = 16 the 16 with the smallest first are listed, in order, and the
    other five leave no trace in any box; objects = 21 at min_blob_cells 2 and 0 at 3 — counted over all blobs."""
    c = oi.pairs_case()
    s = gpu_scanner_factory(c.p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, compact)
        for k in (16, 5, 1):
            for mbc, objs in ((2, 21), (3, 0), (1, 21)):
                what = f"pairs, {layout_name(compact)}, k {k}, min_blob_cells {mbc}"
                got = device_objects(s, d_rec, d_off, d_sd, compact, k, mbc, 17)
                want = oi.hand_want(c.hand, k, mbc)
                want["objects"][:] = objs                                    # not the listed ones alone
                assert_outputs(got, want, what, c.p, 17)
                assert got["objects"].tolist() == [objs] and got["flags"].tolist() == [int(objs >= 17)], what
                assert got["list"]["x1"][0].tolist() == [2 + 3 * i for i in range(k)], what


# ------------------------------------------------------------------ 4. word seams for ranks above 0

def test_word_seams_for_ranks_above_0(gpu_scanner_factory):
    """2000 x 9: three bars of different length, each across a 64-column seam, and a larger blob elsewhere: ranks 1 .. 3
    carry the bars' whole boxes."""
    c = oi.seams_case()
    s = gpu_scanner_factory(c.p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, compact)
        for k in (16, 4, 2):
            what = f"seams, {layout_name(compact)}, k {k}"
            got = device_objects(s, d_rec, d_off, d_sd, compact, k, 12, 3)
            assert_outputs(got, oi.hand_want(c.hand, k, 12), what, c.p, 3)
            assert got["objects"].tolist() == [3] and got["flags"].tolist() == [1], what


# ------------------------------------------------------------------ 5. the sweep on `objects`

def test_objects_through_the_sweep_is_flags_through_the_merge(gpu_scanner_factory):
    """E: clusters_needed 1, three streams, levels 1, 2, 4: mtgpu_sweep_streams_device on `objects` ==
    mtgpu_merge_streams_device on flags at min_objects = L, byte for byte.  F: raising min_blob_cells raises no objects[f]
    and leaves the list alone."""
    import torch
    p, mv, off, sd, pts, soff = oi.streams_case()
    s = gpu_scanner_factory(p)
    CAP = 16
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    d_pts, d_soff = torch.from_numpy(pts.copy()).cuda(), tb.soff_tensor(soff)
    mps = [m.MergeParams(duration=oi.STREAM_FRAMES / oi.FPS, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0) for _ in range(oi.STREAMS)]
    d_mp = torch.from_numpy(np.concatenate([x.to_record() for x in mps]).view(np.uint8).copy()).cuda()
    levels = list(oi.SWEEP_LEVELS)
    res = objects.scan_device(s, d_rec, d_off, d_sd, 16, oi.SWEEP_MIN_BLOB, 1, compact=True)
    assert res["objects"].cpu().numpy().view(np.uint32).tolist() == oi.stream_objects().tolist()
    sseg, sres = s.sweep_streams_device(res["objects"], d_pts, d_soff, d_mp, levels, seg_cap=CAP)
    torch.cuda.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)        # noqa: E731
    kept = []
    for li, lv in enumerate(levels):
        fl = objects.scan_device(s, d_rec, d_off, d_sd, 16, oi.SWEEP_MIN_BLOB, lv, compact=True, want=("flags",))["flags"]
        seg, r8 = s.merge_streams_device(fl, d_pts, d_soff, d_mp, seg_cap=CAP)
        torch.cuda.synchronize()
        assert np.array_equal(bits(sseg[li].cpu().numpy()), bits(seg.cpu().numpy())), lv
        assert np.array_equal(sres[li].cpu().numpy(), r8.cpu().numpy()), lv
        kept.append(int(fl.sum()))
    assert kept == [int((oi.stream_objects() >= lv).sum()) for lv in levels] and kept[0] > kept[1] > kept[2] > 0
    # F
    base = to_host(res)
    want = om.model_batch(p, mv, off, sd, 16, oi.SWEEP_MIN_BLOB)
    assert_outputs(base, want, "three streams", p, 1)
    prev = base["objects"]
    for mbc in (3, 4, 5):
        got = device_objects(s, d_rec, d_off, d_sd, True, 16, mbc, 1)
        assert (got["objects"] <= prev).all() and np.array_equal(got["list"], base["list"]), mbc
        assert got["objects"].tolist() == om.objects_at(want, mbc).tolist(), mbc
        prev = got["objects"]
    assert int(prev.max()) == 0


# ------------------------------------------------------------------ 6. the cliff

@pytest.mark.parametrize("k", [16, 1])
def test_last_grid_the_preview_accepts(gpu_scanner_factory, k):
    """The tallest 65-column grid the preview accepts for k entries: a serpentine over the whole grid and twenty runs up
    from the last row, both record forms, against the model; the ranking table ends at the last byte the launch asks for."""
    c = oi.cliff_case(k)
    gh = oi.cliff_rows(k)
    assert objects.preview(c.p, k)["lds_bytes"] == oi.lds_by_hand(65, gh, k) <= oi.MI355X_LDS < oi.lds_by_hand(65, gh + 1, k)
    want = om.model_batch(c.p, c.mv, c.off, c.sd, k, 5)
    assert want["blobs"].tolist() == [1, 20] and want["objects"].tolist() == [1, 17] and int(want["list"]["cells"][1, 0]) == 21
    assert int(want["list"]["y1"][1, 0]) == gh - 39 and int(want["list"]["y1"][1].min()) >= gh - 39
    s = gpu_scanner_factory(c.p)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, compact)
        what = f"cliff 65x{gh}, k {k}, {layout_name(compact)}"
        got = device_objects(s, d_rec, d_off, d_sd, compact, k, 5, 2)
        assert_outputs(got, want, what, c.p, 2)
        assert_identities(got, what, 5)


def test_first_grid_the_preview_refuses_is_refused_by_the_call(gpu_scanner_factory):
    """One more row than the preview accepts for k = 16: MT_ERR_UNSUPPORTED from both entry points with the grid named,
    and no output byte is touched.  The same context still serves the k the grid does fit, if there is one."""
    import torch
    gh = oi.cliff_rows(16) + 1
    p = bi.limit_params(65, gh, vectors_needed=1, clusters_needed=1)
    assert oi.objects_preview_or_none(p, 16) is None
    s = gpu_scanner_factory(p)
    mv, off, sd = bi.batch_of([bp.plane_frame(oi.cells_plane(65, gh, [(1, 1), (2, 1)]), p.block_shift)], 5)
    d_rec, d_off, d_sd = to_device(mv, off, sd, False)
    out = junk_outputs(1, 16)
    fresh = to_host(junk_outputs(1, 16))
    with pytest.raises(m.MtgpuError) as ei:
        objects.scan_device(s, d_rec, d_off, d_sd, 16, 1, 1, out=out)
    torch.cuda.synchronize()
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and f"65x{gh}" in str(ei.value)
    got = to_host(out)
    for name in OUTPUTS:
        assert got[name].tobytes() == fresh[name].tobytes(), name
    with pytest.raises(m.MtgpuError) as ei:
        objects.scan(s, m.FrameBatch(mv, off, None, sd), 16)
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and f"65x{gh}" in str(ei.value)
    if oi.objects_preview_or_none(p, 1) is not None:
        assert device_objects(s, d_rec, d_off, d_sd, False, 1)["list"]["cells"].tolist() == [[2]]


# ------------------------------------------------------------------ 7. the refusals of the device entry point

def test_contract_program_in_c(tmp_path):
    """tests/c/abi_objects_canaries.c: every refusal with the argument named and canary-filled outputs untouched; the
    caller-sized buffers exactly as the header sizes them, from plain C."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_objects_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_objects_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all object buffers respected" in out.stdout


def test_an_output_on_the_host_is_refused(gpu_scanner_factory):
    """Through the Python layer's raw pointers: a list in host memory, k out of range — refused, junk untouched."""
    import torch
    c = oi.hand_case()
    s = gpu_scanner_factory(c.p)
    lib = m.load_library()
    d_rec, d_off, d_sd = to_device(c.mv, c.off, c.sd, False)
    out = junk_outputs(4, 4)
    host_list = np.full((4, 4, 4), JUNK, dtype=np.int32)

    def call(k, lst):
        rc = lib.mtgpu_scan_objects_device(s._ctx, d_rec.data_ptr(), 40, len(c.mv), d_off.data_ptr(), d_sd.data_ptr(), 4, None, 0, None, k,
                                           1, 1, out["flags"].data_ptr(), out["centres"].data_ptr(), out["blobs"].data_ptr(),
                                           out["objects"].data_ptr(), lst, None)
        torch.cuda.synchronize()
        return rc, lib.mtgpu_last_error().decode()

    for k, lst, word in ((4, host_list.ctypes.data, "d_list is not memory of device"), (0, out["list"].data_ptr(), "k is 0"),
                         (17, out["list"].data_ptr(), "k is 17"), (4, out["list"].data_ptr() + 8, "d_list must be 16-byte aligned")):
        rc, msg = call(k, lst)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (k, msg)
        fresh = to_host(junk_outputs(4, 4))
        got = to_host(out)
        for name in OUTPUTS:
            assert got[name].tobytes() == fresh[name].tobytes(), (word, name)
        assert (host_list == JUNK).all()
    rc, msg = call(4, out["list"].data_ptr())
    assert rc == _abi.MT_OK, msg
    assert_outputs(to_host(out), oi.hand_want(c.hand["plain"], 4), "after the refusals", c.p)


# ------------------------------------------------------------------ 8. example and command

def test_plain_c_objects_example(tmp_path):
    """examples/objects_example.c: a truck, rain and a person, from plain C in a child process (it checks its own numbers)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "objects_example")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "objects_example.c"), "-o", exe, "-L" + pkg, "-lmtgpu",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame 5: 10 centres in 2 blobs, 1 objects: 8 cells at (40, 30) .. (43, 31), 2 cells at (20, 10) .. (21, 10)\n" in out.stdout
    assert ("frame 25: 13 centres in 3 blobs, 2 objects: 8 cells at (40, 30) .. (43, 31), 3 cells at (85, 20) .. (85, 22), "
            "2 cells at (20, 10) .. (21, 10)\n") in out.stdout
    assert "motion frames: 20 of 60 with MIN_OBJECTS 2 at MIN_BLOB_CELLS 3" in out.stdout


def test_end_to_end_command(gpu_scanner_factory, tmp_path, capsys):
    """A .mtmv of the sweep input's first stream, then `python -m mvtrim_amd.objects --json` in a fresh child process and
    the table form in this one: per MIN_OBJECTS level the frames kept, and the two histograms."""
    p, mv, off, sd, pts, soff = oi.streams_case()
    F = oi.STREAM_FRAMES
    frames = [mv[int(off[f]):int(off[f + 1])] for f in range(F)]
    path = str(tmp_path / "stream.mtmv")
    m.mvfile.write_mtmv(path, 1920, 1080, 1, 25, 25.0, F / 25.0, list(range(F)), frames)
    batch, fpts, hdr = tune.load(path)
    assert batch.n_frames == F and hdr["width"] == 1920
    s = gpu_scanner_factory(p)
    mp = m.MergeParams(duration=F / 25.0, max_gap_sec=0.1, padding_sec=0.04, min_savings_pct=5.0)
    direct = objects.measure(s, batch, fpts, [1, 2, 4], mp, 16, 2)
    per_frame = oi.stream_objects()[:F]
    assert [r["motion_frames"] for r in direct["levels"]] == [int((per_frame >= lv).sum()) for lv in (1, 2, 4)] == [18, 12, 6]
    assert direct["objects_per_frame"] == {"0": 6, "1": 6, "2": 3, "3": 3, "4": 3, "5": 3, "6": 0, "7": 0, "8": 0, "9+": 0}
    assert direct["largest_blob"] == 4
    assert direct["listed_sizes"]["2-3"] + direct["listed_sizes"]["4-7"] == int(per_frame.sum()) and direct["listed_sizes"]["1"] == 0
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = [path, "--vectors-needed", "1", "--max-gap-sec", "0.1", "--padding-sec", "0.04", "--min-savings-pct", "5", "--min-blob-cells", "2"]
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.objects"] + args + ["--min-objects", "1,2,4", "--json"], capture_output=True,
                         text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    doc = json.loads(out.stdout)
    assert doc["levels"] == direct["levels"] and doc["objects_per_frame"] == direct["objects_per_frame"]
    assert doc["listed_sizes"] == direct["listed_sizes"] and doc["top"] == 16 and doc["min_blob_cells"] == 2
    assert doc["levels"][0]["seconds_kept"] >= doc["levels"][1]["seconds_kept"] >= doc["levels"][2]["seconds_kept"] > 0.0
    # an object of at least 4 cells: only the third blob of a frame is one
    capsys.readouterr()
    assert objects.main(args[:-1] + ["4", "--top", "2"]) == 0
    text = capsys.readouterr().out
    assert "objects per frame:" in text and "sizes of the listed blobs (top 2):" in text and "MIN_OBJECTS" in text
    assert "an object has at least 4 cells" in text
