"""CPU tier: the motion blobs (include/mtgpu_blobs.h) exist at every layer — header, library, ctypes table, Python
package, command, example — size their launch with host arithmetic alone and reject bad arguments before any HIP call;
the numpy restatement (tests/blobs_model.py) counts the centres the unchanged oracle counts, labels as scipy labels
where scipy imports, and returns every hand-derived number of tests/blobs_inputs.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, blobs, config

import blobs_inputs as bi
import blobs_model as bm
import oracle_binding as ob
import zones_inputs as zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_blobs_preview", "mtgpu_scan_blobs_device", "mtgpu_scan_frames_blobs"]


def blobs_header():
    return open(os.path.join(ROOT, "include", "mtgpu_blobs.h")).read()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = blobs_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_BLOBS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_BLOBS[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        at = hdr.index("int " + n + "(")          # every declaration names the reference lines it stands for
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert "src/motion_scanner.cpp:272-294" in hdr
    assert C.sizeof(_abi.BlobsPlanC) == 16
    assert [f for f, _ in _abi.BlobsPlanC._fields_] == ["lds_bytes", "workgroup", "keep_words_per_row", "keep_words_per_stream"]
    assert _abi.BLOB_BOX_DTYPE.itemsize == 8 and _abi.BLOB_BOX_DTYPE.names == ("x0", "y0", "x1", "y1")
    assert '#include "mtgpu_blobs.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # the header states the consequences the GPU tests rest on, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("min_blob_cells <= 1: flags equals the flags of mtgpu_scan_centres_device", "blobs == 0 <=> centres == 0 <=> largest == 0",
                 "largest <= centres", "blobs largest >= centres", "One scan answers every MIN_BLOB_CELLS", "no pipe form",
                 "components of centre cells, not of active cells"):
        assert text in flat, text
    src = open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "blobs_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"blobs_frames_kernel" in blob and b"blobs_clear_kernel" in blob


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_blobs_plan p;\n"
            "  mt_blob_box b = {0, 0, 0, 0};\n"
            "  return mtgpu_blobs_preview(0, 163840, &p)\n"
            "       + mtgpu_scan_blobs_device(c, 0, 40, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, &b, 0)\n"
            "       + mtgpu_scan_frames_blobs(c, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, &b)\n"
            "       + p.lds_bytes + p.workgroup + p.keep_words_per_row + p.keep_words_per_stream + b.x0 + b.y0 + b.x1 + b.y1\n"
            "       + (int)sizeof(mt_blob_box);\n}\n")
    for first in ("mtgpu.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/blobs_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "blobs_example.c")])


def test_package_exports_the_methods():
    for name in ("scan_blobs", "scan_blobs_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.blobs_preview) and "blobs_preview" in m.__all__
    for name in ("main", "measure", "parser", "histogram"):
        assert callable(getattr(blobs, name)), name


# ------------------------------------------------------------------ preview

def preview(params, lds=MI355X_LDS):
    p = _abi.BlobsPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_blobs_preview(C.byref(c), lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def test_preview_sizes_the_launch_and_the_three_grids_fit():
    # (width, height, kwargs) -> (gw, gh, analysed rows); the first three are the grids that must fit
    for (w, h, kw), (gw, gh, R) in [((1920, 1080, config.CODE_DEFAULTS), (120, 68, 62)), ((3840, 2160, config.CODE_DEFAULTS), (240, 135, 123)),
                                     ((3840, 2160, dict(vertical_mask=0.0)), (240, 135, 135)), ((1280, 720, {}), (80, 45, 41)),
                                     ((48, 48, dict(vertical_mask=0.0)), (3, 3, 3)), ((1920, 1080, dict(vertical_mask=0.5)), (120, 68, 1))]:
        params = m.ScanParams.from_config(w, h, **kw)
        assert (params.grid_w, params.grid_h) == (gw, gh)
        assert max(1, gh - 2 * params.vertical_margin) == R
        rc, p, msg = preview(params)
        assert rc == _abi.MT_OK, msg
        W = (gw + 63) // 64
        assert (p.keep_words_per_row, p.keep_words_per_stream, p.workgroup) == (W, gh * W, 1024)
        assert p.lds_bytes == bi.lds_by_hand(gw, R) <= MI355X_LDS
        assert m.blobs_preview(params) == {"lds_bytes": p.lds_bytes, "workgroup": 1024, "keep_words_per_row": W,
                                           "keep_words_per_stream": gh * W}
        # without the unmasked plane the layout needs less than the masked scan's
        assert p.lds_bytes < m.zones_preview(params)["lds_bytes"]
    assert m.zones_preview(m.ScanParams.from_config(3840, 2160, vertical_mask=0.0))["lds_bytes"] == 144624
    assert bi.lds_by_hand(240, 135) == 140256
    # the grids the plain scan cuts into row bands have no form; nor has 1080p on a device with 16 KB
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    rc, _, msg = preview(m.ScanParams.from_config(1920, 1080), 16384)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg
    with pytest.raises(m.MtgpuError) as ei:
        m.blobs_preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
    lib = m.load_library()
    c = m.ScanParams.from_config(1920, 1080).to_c()
    assert lib.mtgpu_blobs_preview(None, MI355X_LDS, C.byref(_abi.BlobsPlanC())) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_blobs_preview(C.byref(c), MI355X_LDS, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_blobs_preview(C.byref(c), 100, C.byref(_abi.BlobsPlanC())) == _abi.MT_ERR_INVALID


def test_one_more_row_or_column_past_the_limit_is_unsupported():
    shapes = bi.limit_shapes()
    for kind, (gw, gh) in shapes.items():
        rc, p, msg = preview(bi.limit_params(gw, gh))
        assert rc == _abi.MT_OK and p.lds_bytes == bi.lds_by_hand(gw, gh) <= MI355X_LDS, (kind, msg)
        gw2, gh2 = (gw, gh + 1) if kind == "tall" else (gw + 1, gh)
        assert bi.lds_by_hand(gw2, gh2) > MI355X_LDS
        rc, _, msg = preview(bi.limit_params(gw2, gh2))
        assert rc == _abi.MT_ERR_UNSUPPORTED and f"{gw2}x{gh2}" in msg, (kind, msg)
    assert shapes["tall"][0] == 65 and shapes["wide"][1] == 3 and shapes["tall"][1] > 500 and shapes["wide"][0] > 5000


# ------------------------------------------------------------------ error paths that need no device

def test_invalid_arguments_are_rejected_without_a_device():
    """Everything the arguments alone decide is answered before the context is looked at: no HIP call, no byte written."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(64)          # never dereferenced
    odd = C.c_void_p(68)

    def err():
        return lib.mtgpu_last_error().decode()

    def dev(rec=one, rb=40, nrec=1, off=one, n=1, soff=one, ns=1, keep=one, fl=one, ce=one, bl=one, lg=one, bx=one):
        return lib.mtgpu_scan_blobs_device(None, rec, rb, nrec, off, None, n, soff, ns, keep, 1, fl, ce, bl, lg, bx, None)

    for rb in (0, 7, 16, 39, 41, -8):
        assert dev(rb=rb) == inv and "rec_bytes" in err()
    assert dev(fl=None, ce=None, bl=None, lg=None, bx=None) == inv and "all NULL" in err()
    assert dev(off=None) == inv and "d_frame_off" in err()
    assert dev(soff=None) == inv and "d_stream_off" in err()
    assert dev(ns=0) == inv and "n_streams" in err()
    assert dev(keep=None) == inv and "d_keep" in err()                       # stream_off and n_streams without a mask
    assert dev(keep=None, soff=None) == inv and "n_streams" in err()
    assert dev(keep=None, ns=0) == inv and "d_stream_off" in err()
    assert dev(off=odd) == inv and "d_frame_off" in err() and "aligned" in err()
    assert dev(soff=odd) == inv and "d_stream_off" in err() and "aligned" in err()
    assert dev(keep=odd) == inv and "d_keep" in err() and "aligned" in err()
    assert dev(rec=None) == inv and "d_rec" in err()
    assert dev(rec=odd, rb=8) == inv and "d_rec" in err() and "8-byte" in err()
    assert dev(rec=C.c_void_p(66)) == inv and "d_rec" in err()
    assert dev(ce=C.c_void_p(66)) == inv and "d_centres" in err()
    assert dev(bl=C.c_void_p(66)) == inv and "d_blobs" in err()
    assert dev(lg=C.c_void_p(66)) == inv and "d_largest" in err()
    assert dev(bx=C.c_void_p(65)) == inv and "d_box" in err()
    assert dev() == inv and "ctx" in err()
    assert dev(keep=None, soff=None, ns=0) == inv and "ctx" in err()         # the form without a mask is a valid one

    out = np.full(3, 7, dtype=np.uint32)
    fl = np.full(3, 7, dtype=np.uint8)
    box = np.full((3, 4), 7, dtype=np.uint16)
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    keep = np.zeros(4, dtype=np.uint64)
    good_off, good_soff = np.array([0, 4, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)

    def host(off=good_off, soff=good_soff, ns=1, k=keep, f=fl, c=out, b=box, recs=mv):
        return lib.mtgpu_scan_frames_blobs(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(k), 1, vp(f), vp(c), None, None, vp(b))

    assert host(f=None, c=None, b=None) == inv and "all NULL" in err()
    assert host(soff=None) == inv and "stream_off" in err()
    assert host(off=None) == inv and "frame_off" in err()
    assert host(ns=0) == inv and "n_streams" in err()
    assert host(k=None) == inv and "keep is NULL" in err()
    assert host(k=None, soff=None) == inv and "n_streams" in err()
    assert host(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert host(soff=np.array([0, 2, 1], dtype=np.uint64), ns=2) == inv and "stream_off not monotonic" in err()
    assert host(soff=np.array([0, 1], dtype=np.uint64)) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(recs=None) == inv and "mv is NULL" in err()
    assert host() == inv and "ctx" in err()
    assert host(k=None, soff=None, ns=0) == inv and "ctx" in err()
    assert out.tolist() == [7, 7, 7] and fl.tolist() == [7, 7, 7] and (box == 7).all()


# ------------------------------------------------------------------ the model against the oracle and scipy

def all_cases():
    """(name, Case) of every input with records or masks that the GPU tier runs on small grids."""
    out = [("edge columns", bi.edge_columns_case()), ("halo row", bi.halo_row_case()), ("late merges", bi.late_merge_case()),
           ("serpentine 66x12", bi.serpentine_case("66x12")), ("spiral", bi.serpentine_case("spiral")),
           ("dominoes 1080p", bi.domino_case("1080p")), ("tie", bi.tie_case()), ("plumbing", bi.plumbing_case())]
    out += [(f"seam {gw}", bi.seam_case(gw)) for gw in bi.SEAM_GW]
    return out


def test_model_centres_equal_the_oracle():
    """Without a mask: ob.scan_centres on every input.  With masks and vn >= 1: the oracle on filtered records
    (zones_inputs.oracle_batch)."""
    for name, c in all_cases() + [("everything 6", bi.everything_case(6)), ("serpentine 4k", bi.serpentine_case("4k")),
                                  ("limit tall", bi.limit_case("tall")), ("limit wide", bi.limit_case("wide"))]:
        got = bm.model_batch(c.p, c.mv, c.off, c.sd)["centres"]
        assert got.tolist() == ob.scan_centres(c.p, c.mv, c.off, c.sd, nthreads=4)[1].tolist(), name
        if c.keeps is not None and (c.p.vectors_needed & 0xFF) >= 1:
            got = bm.model_batch(c.p, c.mv, c.off, c.sd, c.soff, c.keeps)["centres"]
            assert got.tolist() == zi.oracle_batch(c.p, c.mv, c.off, c.sd, c.soff, c.keeps)[1].tolist(), name


@pytest.mark.parametrize("i", range(len(zi.RANDOM_CASES)))
def test_model_centres_equal_the_oracle_on_the_random_inputs(i):
    p, mv, off, sd, soff, keeps = zi.random_case(i)
    fl, oc, oca = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    masked, plain = bm.model_batch(p, mv, off, sd, soff, keeps), bm.model_batch(p, mv, off, sd)
    assert masked["centres"].tolist() == oc.tolist()
    assert plain["centres"].tolist() == ob.scan_centres(p, mv, off, sd, nthreads=4)[1].tolist()
    for r in (masked, plain):
        c, b, g = (r[k].astype(np.int64) for k in ("centres", "blobs", "largest"))
        assert ((b == 0) == (c == 0)).all() and ((g == 0) == (c == 0)).all() and (g <= c).all() and (b * g >= c).all()
    assert int(plain["blobs"].max()) >= 4 and int(plain["largest"].max()) >= 4          # the inputs label something


def test_model_labels_as_scipy_does():
    ndimage = pytest.importorskip("scipy.ndimage")
    four = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    planes = [bm.centre_plane(c.p, c.mv[int(c.off[f]):int(c.off[f + 1])]) for _, c in all_cases() for f in range(len(c.off) - 1)]
    rng = np.random.RandomState(4)
    planes += [rng.rand(40, 70) < d for d in (0.3, 0.5, 0.6, 0.7)]
    for cen in planes:
        lab, n = ndimage.label(cen, structure=four)
        mine = bm.label(cen)
        assert int(mine.max()) == n
        # the same partition: the pairs (scipy label, model label) are a bijection
        pairs = set(zip(lab[cen].tolist(), mine[cen].tolist()))
        assert len(pairs) == n and len({a for a, _ in pairs}) == n and len({b for _, b in pairs}) == n
        assert not mine[~cen].any()


# ------------------------------------------------------------------ the hand-derived numbers

def assert_hand(c, hand, soff=None, keeps=None, what=""):
    got = bm.model_batch(c.p, c.mv, c.off, c.sd, soff, keeps)
    for k in ("centres", "blobs", "largest"):
        assert got[k].tolist() == hand[k], (what, k, got[k].tolist(), hand[k])
    assert [tuple(b) for b in got["box"].tolist()] == hand["box"], (what, got["box"].tolist(), hand["box"])


def test_every_hand_value_holds_on_the_model():
    for name, c in all_cases():
        if name == "plumbing":
            assert_hand(c, c.hand["plain"], what="plumbing, no mask")
            assert_hand(c, c.hand["masked"], c.soff, c.keeps, what="plumbing, masks")
        elif name.startswith("seam"):
            assert_hand(c, c.hand, c.soff, c.keeps, what=name)
            one = {k: [v[0]] * len(v) for k, v in c.hand.items()}           # keep NULL: one blob again
            assert_hand(c, one, what=name + ", no mask")
            assert all(b == 1 for b in one["blobs"]) and 2 in c.hand["blobs"]
        else:
            assert_hand(c, c.hand, c.soff, c.keeps, what=name)
    for margin in (6, 0):
        assert_hand(bi.everything_case(margin), bi.everything_case(margin).hand, what=f"everything, margin {margin}")
    assert bi.everything_case(6).hand["largest"] == [29274] and bi.everything_case(6).hand["box"] == [(1, 6, 238, 128)]
    assert_hand(bi.serpentine_case("4k"), bi.serpentine_case("4k").hand, what="serpentine 4k")
    assert_hand(bi.domino_case("4k"), bi.domino_case("4k").hand, what="dominoes 4k")
    assert bi.serpentine_case("66x12").hand["largest"] == [389]
    assert bi.domino_case("1080p").hand["blobs"][0] > 1024 and bi.domino_case("4k").hand["blobs"][0] > 4096


def test_thin_paths_are_thin():
    """The serpentine's joints and the spiral: no cell of the spiral has more than two neighbours on it, so the path is
    as long as its cell count — the input that a one-cell-per-round propagation needs thousands of rounds for."""
    cells = bi.spiral_cells(1, 3, 118, 64)
    on = set(cells)
    assert max(sum((x + dx, y + dy) in on for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))) for x, y in cells) == 2
    assert sum(1 for x, y in cells if sum((x + dx, y + dy) in on for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))) == 1) == 2
    assert len(cells) > 3000


def test_sweep_input_separates_the_two_rules():
    p, mv, off, sd, pts, soff = bi.sweep_case()
    r = bm.model_batch(p, mv, off, sd)
    assert sorted(set(r["largest"].tolist())) == [2, 4, 9] and sorted(set(r["centres"].tolist())) == [8, 10, 12, 17]
    for lv in bi.SWEEP_LEVELS:
        by_blob, by_cell = int((r["largest"] >= lv).sum()), int((r["centres"] >= lv).sum())
        assert by_cell == 96 and by_blob == {1: 96, 2: 96, 4: 48, 8: 24}[lv]


# ------------------------------------------------------------------ the command

def test_blobs_options_parse():
    a = blobs.parser().parse_args(["f.mtmv", "--min-blob-cells", "1,3,9", "--keep", "cam.mtkeep", "--json", "--width", "1920",
                                   "--height", "1080", "--duration", "12.5", "--vertical-mask", "0", "--vectors-needed", "3"])
    assert a.min_blob_cells == [1, 3, 9] and a.keep == "cam.mtkeep" and a.json
    assert (a.width, a.height, a.duration, a.vertical_mask, a.vectors_needed) == (1920, 1080, 12.5, 0.0, 3)
    a = blobs.parser().parse_args(["f"])
    assert a.min_blob_cells == [1, 2, 4, 8] and a.keep is None and not a.json
    assert blobs.histogram(np.array([0, 0, 1, 3, 9, 12, 200], dtype=np.uint32)) == {
        "0": 2, "1": 1, "2": 0, "3": 1, "4": 0, "5": 0, "6": 0, "7": 0, "8": 0, "9+": 3}


@pytest.mark.parametrize("bad", [
    ["--min-blob-cells", ""], ["--min-blob-cells", "a"], ["--min-blob-cells", "1,,2"], ["--min-blob-cells", "0"],
    ["--min-blob-cells", "-3"], ["--min-blob-cells", "1.5"], ["--min-blob-cells", "2,2"], ["--min-blob-cells", "4294967296"],
    ["--min-blob-cells", ",".join(str(i) for i in range(1, 18))], ["--width", "x"], ["--device", "gpu"], ["--keep"],
])
def test_blobs_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(blobs, "MotionScanner", boom)
    monkeypatch.setattr(blobs.tune, "load", boom)
    monkeypatch.setattr(blobs.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        blobs.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_blobs_missing_geometry_exits_2_bad_mask_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(blobs, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height / duration
    with pytest.raises(SystemExit) as ei:
        blobs.main([path])
    assert ei.value.code == 2
    from mvtrim_amd import zones
    zones.save_keep(str(tmp_path / "wrong.mtkeep"), np.ones((3, 3), dtype=bool))
    with pytest.raises(SystemExit) as ei:
        blobs.main([path, "--width", "160", "--height", "160", "--duration", "1", "--keep", str(tmp_path / "wrong.mtkeep")])
    assert ei.value.code == 2
    assert blobs.main([str(tmp_path / "nothing_here.json")]) == 1
    assert blobs.main([path, "--width", "160", "--height", "160", "--duration", "1", "--keep", str(tmp_path / "none.mtkeep")]) == 1
