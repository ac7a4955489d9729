"""CPU tier: the ignore zones (include/mtgpu_zones.h) exist at every layer — header, library, ctypes table, Python
package, command, example — size their launch with host arithmetic alone, reject bad arguments before any HIP call and
have no fallback without a device; the mask helpers of zones.py are plain numpy; and every hand-derived number of
tests/zones_inputs.py equals the oracle on filtered records (vectors_needed >= 1) and the numpy restatement of the AND
rule (every vectors_needed)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, config, zones

import np_model
import oracle_binding as ob
import zones_inputs as zi
from golden_cases import load_hand_cases
import derived_edge_inputs as dei

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_scan_frames_zones", "mtgpu_scan_zones_device", "mtgpu_zones_preview"]


def zones_header():
    return open(os.path.join(ROOT, "include", "mtgpu_zones.h")).read()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = zones_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_ZONES)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_ZONES[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        # every declaration names the reference lines it stands for
        at = hdr.index("int " + n + "(")
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert C.sizeof(_abi.ZonesPlanC) == 16
    assert [f for f, _ in _abi.ZonesPlanC._fields_] == ["lds_bytes", "workgroup", "keep_words_per_row", "keep_words_per_stream"]
    # mtgpu.h hands the declarations to everyone who includes it
    assert '#include "mtgpu_zones.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # the header states both vn == 0 facts
    flat = " ".join(hdr.replace("*", " ").split())
    assert "deliberately NOT record removal" in flat and "margin equivalence does NOT hold for vn == 0" in flat
    # no new environment variable
    assert "getenv" not in open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "zones_kernels.hip")).read()
    # the kernels are in the library, and nothing of the checker is
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"zones_frames_kernel" in blob and b"zones_clear_kernel" in blob
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    assert "mto_" not in syms


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_zones_plan p;\n"
            "  return mtgpu_zones_preview(0, 163840, &p)\n"
            "       + mtgpu_scan_zones_device(c, 0, 40, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0)\n"
            "       + mtgpu_scan_frames_zones(c, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0)\n"
            "       + p.lds_bytes + p.workgroup + p.keep_words_per_row + p.keep_words_per_stream;\n}\n")
    for first in ("mtgpu.h", "mtgpu_zones.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/zones_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "zones_example.c")])


def test_package_exports_the_methods():
    for name in ("scan_zones", "scan_zones_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.zones_preview) and "zones_preview" in m.__all__
    for name in ("pack_keep", "unpack_keep", "keep_from_rects", "keep_from_activity", "main", "measure", "parser"):
        assert callable(getattr(zones, name)), name


# ------------------------------------------------------------------ preview

def preview(params, lds=MI355X_LDS):
    p = _abi.ZonesPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_zones_preview(C.byref(c), lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def lds_by_hand(gw, R):
    """csrc/zones_kernels.h: the tile, R keep rows, two planes of R + 2 mask rows, 16 bytes of totals."""
    W = (gw + 63) // 64
    return 4 * (((R + 2) * gw + 3) & ~3) + (3 * R + 4) * W * 8 + 16


def test_preview_sizes_the_launch_and_the_mask():
    # (width, height, kwargs) -> (gw, gh, analysed rows)
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
        assert p.lds_bytes == lds_by_hand(gw, R) <= MI355X_LDS
        assert m.zones_preview(params) == {"lds_bytes": p.lds_bytes, "workgroup": 1024, "keep_words_per_row": W,
                                           "keep_words_per_stream": gh * W}
    # about 32 KB at 1080p: two workgroups of 1024 lanes per CU are limited by lanes, not LDS; 4K sits alone on its CU
    assert 2 * preview(m.ScanParams.from_config(1920, 1080))[1].lds_bytes <= MI355X_LDS
    assert 2 * preview(m.ScanParams.from_config(3840, 2160))[1].lds_bytes > MI355X_LDS
    # the grids the plain scan cuts into row bands have no form; nor has 1080p on a device with 32 KB
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    rc, _, msg = preview(m.ScanParams.from_config(1920, 1080), 32768)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg
    with pytest.raises(m.MtgpuError) as ei:
        m.zones_preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
    # invalid
    lib = m.load_library()
    c = m.ScanParams.from_config(1920, 1080).to_c()
    assert lib.mtgpu_zones_preview(None, MI355X_LDS, C.byref(_abi.ZonesPlanC())) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_zones_preview(C.byref(c), MI355X_LDS, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_zones_preview(C.byref(c), 100, C.byref(_abi.ZonesPlanC())) == _abi.MT_ERR_INVALID


# ------------------------------------------------------------------ error paths that need no device

def test_invalid_arguments_are_rejected_without_a_device():
    """Everything the arguments alone decide is answered before the context is looked at: no HIP call, no byte written."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(64)          # never dereferenced
    odd = C.c_void_p(68)

    def err():
        return lib.mtgpu_last_error().decode()

    def dev(rec=one, rb=40, nrec=1, off=one, n=1, soff=one, ns=1, keep=one, fl=one, ce=one, ca=one):
        return lib.mtgpu_scan_zones_device(None, rec, rb, nrec, off, None, n, soff, ns, keep, fl, ce, ca, None)

    for rb in (0, 7, 16, 39, 41, -8):
        assert dev(rb=rb) == inv and "rec_bytes" in err()
    assert dev(fl=None, ce=None, ca=None) == inv and "all NULL" in err()
    assert dev(off=None) == inv and "d_frame_off" in err()
    assert dev(soff=None) == inv and "d_stream_off" in err()
    assert dev(keep=None) == inv and "d_keep" in err()
    assert dev(ns=0) == inv and "n_streams" in err()
    assert dev(off=odd) == inv and "d_frame_off" in err() and "aligned" in err()
    assert dev(soff=odd) == inv and "d_stream_off" in err() and "aligned" in err()
    assert dev(keep=odd) == inv and "d_keep" in err() and "aligned" in err()
    assert dev(rec=None) == inv and "d_rec" in err()
    assert dev(rec=odd, rb=8) == inv and "d_rec" in err() and "8-byte" in err()
    assert dev(rec=C.c_void_p(66)) == inv and "d_rec" in err()
    assert dev(ce=C.c_void_p(66)) == inv and "d_centres " in err()
    assert dev(ca=C.c_void_p(66)) == inv and "d_centres_all" in err()
    assert dev() == inv and "ctx" in err()

    out = np.full(3, 7, dtype=np.uint32)
    fl = np.full(3, 7, dtype=np.uint8)
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    keep = np.zeros(4, dtype=np.uint64)
    good_off, good_soff = np.array([0, 4, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)

    def host(off=good_off, soff=good_soff, ns=1, k=keep, f=fl, c=out, a=None, recs=mv):
        return lib.mtgpu_scan_frames_zones(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(k), vp(f), vp(c), vp(a))

    assert host(f=None, c=None) == inv and "all NULL" in err()
    assert host(soff=None) == inv and "stream_off" in err()
    assert host(off=None) == inv and "frame_off" in err()
    assert host(ns=0, soff=np.array([2], dtype=np.uint64)) == inv and "n_streams" in err()
    assert host(k=None) == inv and "keep" in err()
    assert host(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert host(soff=np.array([0, 2, 1], dtype=np.uint64), ns=2) == inv and "stream_off not monotonic" in err()
    assert host(soff=np.array([0, 1], dtype=np.uint64)) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(recs=None) == inv and "mv is NULL" in err()
    assert host() == inv and "ctx" in err()
    assert out.tolist() == [7, 7, 7] and fl.tolist() == [7, 7, 7]


def test_no_fallback_without_a_device(tmp_path):
    """A context cannot be created without a device (MT_ERR_DEVICE, "no CPU fallback"), and the command, given a
    readable file, prints its table with a device and fails with that message without one."""
    mv = np.zeros(4, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"], mv["src_x"], mv["src_y"] = [40, 41, 56, 57], 40, [30, 31, 46, 47], 40
    path = str(tmp_path / "two.mtmv")
    m.mvfile.write_mtmv(path, 160, 160, 1, 1000, 25.0, 1.0, [0, 40], [mv, None])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.zones", path, "--mv-threshold-sq", "4", "--vectors-needed", "2",
                          "--clusters-needed", "1", "--vertical-mask", "0", "--ignore", "32,32,48,48", "--json"],
                         capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    if m.load_library().mtgpu_device_count() > 0:
        # cells (2, 2) and (3, 2) of a 10 x 10 grid hold two votes each: two centres; the rectangle takes cell (2, 2)
        import json
        assert out.returncode == 0, out.stderr
        doc = json.loads(out.stdout)
        assert doc["without_zones"]["centres"] == 2 and doc["with_zones"]["centres"] == 0 and doc["ignored_cells"] == 1
        return
    assert out.returncode != 0 and out.stdout == ""
    assert "no CPU fallback" in out.stderr
    with pytest.raises(m.MtgpuError) as ei:
        m.MotionScanner(m.ScanParams.from_config(160, 160))
    assert ei.value.code == _abi.MT_ERR_DEVICE and "no CPU fallback" in str(ei.value)


# ------------------------------------------------------------------ zones.py

@pytest.mark.parametrize("gw", [1, 63, 64, 65, 128, 129])
def test_pack_and_unpack_round_trip(gw):
    rng = np.random.RandomState(gw)
    keep = rng.rand(5, gw) < 0.5
    keep[0], keep[1] = True, False
    words = zones.pack_keep(keep)
    W = (gw + 63) // 64
    assert words.dtype == np.uint64 and words.shape == (5, W) and words.flags["C_CONTIGUOUS"]
    assert np.array_equal(zones.unpack_keep(words, gw), keep)
    for y in range(5):                                     # the layout of include/mtgpu_zones.h, bit by bit
        for x in range(gw):
            assert bool((int(words[y, x >> 6]) >> (x & 63)) & 1) == bool(keep[y, x])
    full = int(words[0].sum(dtype=np.uint64)) if W == 1 else None
    if W == 1:
        assert full == (1 << gw) - 1                       # bits at x >= gw are 0
    assert int(words[1].sum()) == 0
    junk = words.copy()
    if gw % 64:
        junk[:, -1] |= np.uint64(1) << np.uint64(63)       # a bit at x >= gw is dropped
    assert np.array_equal(zones.unpack_keep(junk, gw), keep)
    with pytest.raises(ValueError):
        zones.unpack_keep(words, gw + 64)
    with pytest.raises(ValueError):
        zones.pack_keep(np.ones(3, dtype=bool))


def test_rectangles_ignore_every_cell_their_blocks_intersect():
    p = m.ScanParams.from_config(1920, 1080, vertical_mask=0.0)          # 16-pixel blocks, 120 x 68

    def ignored(rects, unit="px", **kw):
        k = zones.keep_from_rects(p, rects, unit, **kw)
        assert k.shape == (68, 120) and k.dtype == bool
        ys, xs = np.nonzero(~k)
        return (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()), int((~k).sum())) if len(xs) else None

    # edges exactly on a block boundary: [32, 64) x [16, 48) is columns 2 .. 3, rows 1 .. 2
    assert ignored([(32, 16, 64, 48)]) == (2, 1, 3, 2, 4)
    # one pixel off: the left edge one pixel earlier takes column 1, the right edge one pixel later takes column 4
    assert ignored([(31, 16, 64, 48)]) == (1, 1, 3, 2, 6)
    assert ignored([(32, 16, 65, 48)]) == (2, 1, 4, 2, 6)
    assert ignored([(33, 17, 63, 47)]) == (2, 1, 3, 2, 4)
    assert ignored([(32, 15, 64, 49)]) == (2, 0, 3, 3, 8)
    assert ignored([(47, 31, 48, 32)]) == (2, 1, 2, 1, 1)                # one pixel, the last of its block
    assert ignored([(48, 32, 48, 40)]) is None and ignored([]) is None  # empty
    assert ignored([(1900, 1070, 5000, 5000)]) == (118, 66, 119, 67, 4)  # clipped to the grid
    assert ignored([(0, 0, 16, 16), (1904, 1072, 1920, 1088)])[4] == 2   # two rectangles
    # cells
    assert ignored([(2, 1, 4, 3)], "cell") == (2, 1, 3, 2, 4)
    # fractions of the picture: floor / ceil in pixels, then as pixels.  The right half of 1920 starts at pixel 960 =
    # column 60; the top tenth of 1080 ends at pixel 108, inside row 6
    assert ignored([(0.5, 0.0, 1.0, 0.1)], "frac", size=(1920, 1080)) == (60, 0, 119, 6, 60 * 7)
    assert ignored([(0.0, 0.0, 1.0, 1.0)], "frac", size=(1920, 1080))[4] == 68 * 120
    assert ignored([(0.25, 0.25, 0.25, 0.5)], "frac") is None
    # without `size` a fraction is of the grid's own extent, 1920 x 1088
    assert ignored([(0.0, 0.5, 1.0, 1.0)], "frac") == (0, 34, 119, 67, 34 * 120)
    for bad in ([(0, 0, 1.5, 1)], [(0.5, 0, 2, 1)]):
        with pytest.raises(ValueError):
            zones.keep_from_rects(p, bad, "frac" if bad[0][2] == 2 else "px")
    with pytest.raises(ValueError):
        zones.keep_from_rects(p, [], "inch")
    # another block size
    p8 = m.ScanParams.from_config(1920, 1080, block_size=8, block_shift=3, vertical_mask=0.0)
    k = zones.keep_from_rects(p8, [(8, 8, 17, 9)])
    assert (~k).sum() == 2 and not k[1, 1] and not k[1, 2]


def test_keep_from_activity_thresholds_and_ties():
    centre = np.array([[0, 1, 5], [10, 9, 4]], dtype=np.uint32)
    assert zones.keep_from_activity(centre, 10, 1.0).all()                # a cell is a centre at most once per frame
    assert np.array_equal(zones.keep_from_activity(centre, 10, 0.0), centre == 0)      # every cell that ever was one
    assert np.array_equal(zones.keep_from_activity(centre, 10, 0.5), [[True, True, True], [False, False, True]])   # 5 == 0.5 x 10 is kept
    assert np.array_equal(zones.keep_from_activity(centre, 10, 0.4), [[True, True, False], [False, False, True]])  # 4 == 0.4 x 10 is kept
    assert zones.keep_from_activity(centre, 0, 0.0).tolist() == (centre == 0).tolist()
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            zones.keep_from_activity(centre, 10, bad)
    k = np.ones((8, 10), dtype=bool)
    k[0, :] = False
    k[3, :5] = False
    assert zones.ignored_share(k, 0) == 15 / 80 and zones.ignored_share(k, 1) == 5 / 60 and zones.ignored_share(k, 4) == 0.0


def test_zones_options_parse():
    a = zones.parser().parse_args(["f.mtmv", "--ignore", "0,0,64,32", "--ignore", "100,200,300,400", "--ignore-busy", "0.9",
                                   "--mask-npy", "in.npy", "--save-mask", "out.npy", "--json", "--width", "1920", "--height", "1080",
                                   "--duration", "12.5", "--vertical-mask", "0", "--vectors-needed", "3"])
    assert a.ignore == [(0.0, 0.0, 64.0, 32.0), (100.0, 200.0, 300.0, 400.0)] and a.ignore_busy == 0.9 and a.unit == "px"
    assert (a.mask_npy, a.save_mask, a.json, a.width, a.height, a.duration) == ("in.npy", "out.npy", True, 1920, 1080, 12.5)
    a = zones.parser().parse_args(["f", "--unit", "frac", "--ignore", "0.5,0,1,0.25"])
    assert a.ignore == [(0.5, 0.0, 1.0, 0.25)] and a.ignore_busy is None and a.mask_npy is None


@pytest.mark.parametrize("bad", [
    ["--ignore", "1,2,3"], ["--ignore", "1,2,3,4,5"], ["--ignore", "a,b,c,d"], ["--ignore", ""], ["--ignore", "0,0,nan,4"],
    ["--ignore", "-1,0,4,4"], ["--ignore", "8,0,4,4"], ["--ignore", "0,8,4,4"], ["--ignore", "0,0,inf,4"],
    ["--ignore", "0.5,0,8,8"], ["--ignore", "0,0,2,1", "--unit", "frac"], ["--unit", "inch"],
    ["--ignore-busy", "-0.1"], ["--ignore-busy", "1.5"], ["--ignore-busy", "x"], ["--ignore-busy", "nan"], ["--ignore-busy", ""],
])
def test_zones_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    """argparse's exit code 2, and neither the file nor a scanner has been looked at."""
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(zones, "MotionScanner", boom)
    monkeypatch.setattr(zones.tune, "load", boom)
    monkeypatch.setattr(zones.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        zones.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_zones_missing_geometry_exits_2_bad_mask_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(zones, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height / duration
    with pytest.raises(SystemExit) as ei:
        zones.main([path])
    assert ei.value.code == 2
    np.save(str(tmp_path / "wrong.npy"), np.ones((3, 3), dtype=bool))
    with pytest.raises(SystemExit) as ei:
        zones.main([path, "--width", "160", "--height", "160", "--duration", "1", "--mask-npy", str(tmp_path / "wrong.npy")])
    assert ei.value.code == 2
    assert zones.main([str(tmp_path / "nothing_here.json")]) == 1
    assert zones.main([path, "--width", "160", "--height", "160", "--duration", "1", "--mask-npy", str(tmp_path / "none.npy")]) == 1


# ------------------------------------------------------------------ the hand-derived numbers

def test_model_equals_np_model_and_the_oracle_without_a_mask():
    """The restatement itself: with a full mask both of its counts are np_model's and the oracle's, on the 30
    hand-derived check_frame cases (vectors_needed 0 and a margin included)."""
    _, cases = load_hand_cases()
    assert len(cases) == 30
    for name, kw, case in cases:
        mv, off, sd, hand = dei.hand_case_batch(case)
        for vn in (kw["vectors_needed"], 0, 255):
            p = m.ScanParams.from_config(**dict(kw, vectors_needed=vn))
            want = np_model.check_frame_np(p, mv, True)[1]
            assert zi.zone_counts_np(p, mv, np.ones((p.grid_h, p.grid_w), dtype=bool)) == (want, want), (name, vn)
            assert int(ob.scan_centres(p, mv, off, np.ones(1, dtype=np.uint8))[1][0]) == want, (name, vn)
            if vn == kw["vectors_needed"] and sd[0]:
                assert want == hand, name


def test_word_seam_hand_values():
    p, mv, off, sd, soff, keeps, hand, hand_all = zi.seam_case()
    assert (p.grid_w + 63) // 64 == 3 and len(hand) == 14
    c, ca = zi.model_batch(p, mv, off, sd, soff, keeps)
    assert c.tolist() == hand.tolist() and ca.tolist() == hand_all.tolist()
    fl, oc, oca = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert oc.tolist() == hand.tolist() and oca.tolist() == hand_all.tolist() and fl.tolist() == [1 if v else 0 for v in hand]
    # what a carry read from the UNMASKED neighbour word would return differs from the hand value on frame B
    assert hand.tolist()[3] == 2 and hand.tolist()[5] == 2 and hand_all.tolist()[3] == 4


@pytest.mark.parametrize("margin", [0, 1])
def test_vectors_needed_zero_hand_values(margin):
    p, off, sd, soff, keeps, hand, hand_all = zi.vn0_case(margin)
    none = np.zeros(0, dtype=m.MV_DTYPE)
    c, ca = zi.model_batch(p, none, off, sd, soff, keeps)
    assert c.tolist() == hand.tolist() and ca.tolist() == hand_all.tolist()
    # the unmasked count is the reference's (every frame has side data and no record)
    assert ob.scan_centres(p, none, off, sd)[1].tolist() == hand_all.tolist()
    # has_sd == NULL: no record, no side data, 0 everywhere
    c, ca = zi.model_batch(p, none, off, None, soff, keeps)
    assert not c.any() and not ca.any() and not ob.scan_centres(p, none, off, None)[1].any()
    # the margin is no mask with vn == 0: a single kept cell on row 1 has the margin row as an active neighbour under
    # margin 1, and no neighbour at all under margin 0 with rows 0 and 7 cleared
    if margin == 1:
        p0 = zi.vn0_case(0)[0]
        strip = np.ones((1, 8, 10), dtype=bool)
        strip[0, [0, 7]] = False
        single = zi._only([(4, 1)])[None]
        assert zi.model_batch(p0, none, off[:2], sd[:1], soff[:2], single & strip)[0].tolist() == [0]
        assert zi.model_batch(p, none, off[:2], sd[:1], soff[:2], single)[0].tolist() == [1]


def test_stream_lookup_hand_values():
    p, mv, off, sd, soff, keeps, hand, hand_all = zi.lookup_case()
    assert np.diff(soff.astype(np.int64)).tolist() == [0, 1, 2, 0, 3, 1] and len(hand) == 9
    c, ca = zi.model_batch(p, mv, off, sd, soff, keeps)
    assert c.tolist() == hand.tolist() and ca.tolist() == hand_all.tolist()
    fl, oc, oca = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert oc.tolist() == hand.tolist() and oca.tolist() == hand_all.tolist()
    assert fl.tolist() == [int(v >= 4) for v in hand]                   # clusters_needed 4: stream 1's frame stays below
    # the count tells the stream: the streams that own frames give four different values
    assert len({int(hand[int(soff[s])]) for s in (1, 2, 5)} | {int(hand[4])}) == 4


# ------------------------------------------------------------------ counts to count

@pytest.mark.parametrize("i", range(len(zi.RANDOM_CASES)))
def test_random_mask_inputs_hold_centres_and_both_equivalences_hold(i):
    """The numpy model with the AND rule == the oracle on filtered records, and the inputs count something: at least
    half of the frames with records have a non-zero masked count, at least a quarter lose centres to the mask."""
    p, mv, off, sd, soff, keeps = zi.random_case(i)
    c, ca = zi.model_batch(p, mv, off, sd, soff, keeps)
    fl, oc, oca = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert c.tolist() == oc.tolist() and ca.tolist() == oca.tolist()
    assert fl.tolist() == (oc >= 2).astype(np.uint8).tolist()
    assert zi.counts_to_count(c, ca, off, sd)
    a, b = int(soff[3]), int(soff[4])
    assert not c[a:b].any() and ca[a:b][sd[a:b] != 0].all()              # the all-zero mask: every count 0, centres_all not
    assert int(soff[1]) == int(soff[2])                                  # the empty stream
    assert not c[sd == 0].any() and not ca[sd == 0].any()
    assert 0.2 < 1.0 - keeps[[0, 2, 4]].mean() < 0.4


def test_planning_input_holds_centres():
    p, mv, off, sd, soff, keeps = zi.plan_case()
    assert len(off) - 1 == zi.PLAN_FRAMES > 32 * 1024
    fl, oc, oca = zi.oracle_batch(p, mv, off, sd, soff, keeps)
    assert zi.counts_to_count(oc, oca, off, sd)
    sample = np.arange(0, zi.PLAN_FRAMES, 397)
    c, ca = zi.model_batch(p, mv, off, sd, soff, keeps)[0][sample], None
    assert c.tolist() == oc[sample].tolist()
    assert set(np.unique(oca).tolist()) <= {0, 3, 4} and len(np.unique(oc)) >= 3 and 0 < int(fl.sum()) < int((oc > 0).sum())


def test_margin_as_mask_on_the_model():
    """vn >= 1: margin 0 plus a mask that clears rows [0, m) and [gh - m, gh) equals margin m without a mask — and the
    input tells the three margins apart in most frames."""
    mv, off, sd = zi.margin_case()
    p0 = m.ScanParams.from_config(1920, 1080, vertical_mask=0.0)
    counts = [ob.scan_centres(p0, mv, off, sd)[1]]
    for vmask, margin in zi.MARGIN_MASKS:
        pm = m.ScanParams.from_config(1920, 1080, vertical_mask=vmask)
        assert pm.vertical_margin == margin
        strip = np.ones((1, 68, 120), dtype=bool)
        strip[0, :margin] = strip[0, 68 - margin:] = False
        want = ob.scan_centres(pm, mv, off, sd)[1]
        assert zi.model_batch(p0, mv, off, sd, [0, 24], strip)[0].tolist() == want.tolist()
        counts.append(want)
    assert int((counts[0] > counts[1]).sum()) >= 12 and int((counts[1] > counts[2]).sum()) >= 12 and int((counts[2] > 0).sum()) == 24
