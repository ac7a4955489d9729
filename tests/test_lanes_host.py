"""CPU tier: direction planes (include/mtgpu_lanes.h) exist at every layer — header, library, ctypes table, Python package,
command, example — size their launch with host arithmetic alone and reject bad arguments before any HIP call; the plane
helpers of lanes.py and the `.mtdir` file format; and the model of tests/lanes_model.py, which tests/test_gpu_lanes.py
holds the kernels to, equals the unchanged oracle on filtered records (consequence C) and every hand-derived number of
tests/lanes_inputs.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, config, lanes

import dir_model as dm
import lanes_inputs as li
import lanes_model as lm
import oracle_binding as ob
import zones_inputs as zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc")
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_flow_map", "mtgpu_flow_map_device", "mtgpu_lanes_preview", "mtgpu_scan_frames_lanes", "mtgpu_scan_lanes_device"]


def lanes_header():
    return open(os.path.join(ROOT, "include", "mtgpu_lanes.h")).read()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = lanes_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_LANES)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_LANES[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        # every declaration names the reference lines it stands for
        at = hdr.index("int " + n + "(")
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert C.sizeof(_abi.LanesPlanC) == 16
    assert [f for f, _ in _abi.LanesPlanC._fields_] == ["lds_bytes", "workgroup", "staged", "plane_bytes"]
    # mtgpu.h hands the declarations to everyone who includes it: behind the direction filter, ahead of the persistence header
    top = open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert top.index('#include "mtgpu_dir.h"') < top.index('#include "mtgpu_lanes.h"') < top.index('#include "mtgpu_persist.h"')
    assert not any(n in top for n in NEW_SYMBOLS)
    # the header states the semantics, the consequences the tests rest on, the sizes and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("plane[y gw + x] is the allow byte of cell (x, y)", "12 ay <= 5 ax", "A counting record without a sector always votes",
                 "Bytes of cells outside the analysed rows are never read", "d_planes == NULL is MT_ERR_INVALID",
                 "d_flow[((s 8 + k) gh + y) gw + x]", "The call clears, then counts", "A frame outside every stream counts nowhere",
                 "A. A plane filled with one byte b", "B. A plane of 0xFF is mtgpu_scan_centres_device", "C. Removal", "D. Monotone",
                 "E. Zones tie", "F. vn == 0 gives the plain centre scan", "G. For every stream and every k",
                 "31 792", "7 440", "39 232", "124 048", "29 520", "153 568", "135 952", "32 400", "168 352 > 163 840",
                 "Out of scope: the pipe, the C++ host layer and mtgpu_scan_file", "a min_centres filter on the flow map",
                 "MT_ERR_UNSUPPORTED with the grid named"):
        assert text in flat, text
    src = open(os.path.join(CSRC, "lanes_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "#error" in src
    assert "amdgpu_waves_per_eu(8, 8)" in src and "__launch_bounds__(BLOCK)" in src
    # record_stream.h serves the new kernels as it is: the functors live in the new file
    assert "stream_compact<BLOCK, UNROLL>" in src and "stream_mv40<BLOCK, UNROLL>" in src and "lanes_vote" in src and "flow_count" in src
    # the kernels are in the library, and nothing of the checker is
    blob = open(_abi.LIB_PATH, "rb").read()
    for kernel in (b"lanes_frames_kernel", b"lanes_clear_kernel", b"flow_frames_kernel", b"flow_clear_kernel"):
        assert kernel in blob, kernel
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    assert "mto_" not in syms
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lanes_kernels.hip" in mk and "lanes_kernels.h " in mk and "mtgpu_lanes.h" in mk


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_lanes_plan p;\n"
            "  mt_dir_rose r = {{0, 0, 0, 0, 0, 0, 0, 0}};\n"
            "  uint8_t plane[4] = {MTGPU_DIR_ALL, 0, 1, 2};\n"
            "  uint32_t flow[32];\n"
            "  return mtgpu_lanes_preview(0, 163840, &p)\n"
            "       + mtgpu_scan_lanes_device(c, 0, 40, 0, 0, 0, 0, 0, 0, plane, 0, 0, &r, 0)\n"
            "       + mtgpu_scan_frames_lanes(c, 0, 0, 0, 0, 0, 0, plane, 0, 0, &r)\n"
            "       + mtgpu_flow_map_device(c, 0, 40, 0, 0, 0, 0, 0, 0, flow, 0)\n"
            "       + mtgpu_flow_map(c, 0, 0, 0, 0, 0, 0, flow)\n"
            "       + p.lds_bytes + p.workgroup + p.staged + p.plane_bytes;\n}\n")
    for first in ("mtgpu.h", "mtgpu_lanes.h", "mtgpu_dir.h", "mtgpu_persist.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_lanes.h"\n#include "mtgpu_dir.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/lanes_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "lanes_example.c")])


def test_canary_program_builds(tmp_path):
    """The plain-C contract program of the GPU tier compiles and links against the ABI (it cannot run without a device)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_lanes_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_lanes_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_package_exports_the_methods():
    for name in ("scan_lanes", "scan_lanes_device", "flow_map", "flow_map_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.lanes_preview) and "lanes_preview" in m.__all__
    for name in ("plane_from_rects", "plane_from_flow", "invert_plane", "save_plane", "load_plane", "main", "measure", "parser"):
        assert callable(getattr(lanes, name)), name


# ------------------------------------------------------------------ preview

def preview(params, lds=MI355X_LDS):
    p = _abi.LanesPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_lanes_preview(C.byref(c), lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def dir_lds_by_hand(gw, R):
    """csrc/dir_kernels.h: the tile, one plane of R + 2 mask rows, 16 bytes of totals, the eight rose words."""
    W = (gw + 63) // 64
    return 4 * (((R + 2) * gw + 3) & ~3) + (R + 2) * W * 8 + 16 + 32


def rows_by_hand(gw, R):
    """csrc/lanes_kernels.h: the analysed rows of one plane, padded to 16 bytes."""
    return (R * gw + 15) & ~15


def test_preview_sizes_the_launch():
    # the header's table: the direction scan's LDS, the plane's analysed rows, the total, the form
    table = [((1920, 1080, config.CODE_DEFAULTS), (120, 68, 62), 31792, 7440, 39232, 1),
             ((3840, 2160, config.CODE_DEFAULTS), (240, 135, 123), 124048, 29520, 153568, 1),
             ((3840, 2160, dict(vertical_mask=0.0)), (240, 135, 135), 135952, 32400, 135952, 0)]
    for (w, h, kw), (gw, gh, R), base, rows, total, staged in table:
        params = m.ScanParams.from_config(w, h, **kw)
        assert (params.grid_w, params.grid_h, max(1, gh - 2 * params.vertical_margin)) == (gw, gh, R)
        assert dir_lds_by_hand(gw, R) == base == m.dir_preview(params)["lds_bytes"] and rows_by_hand(gw, R) == rows == R * gw
        rc, p, msg = preview(params)
        assert rc == _abi.MT_OK, msg
        assert (p.lds_bytes, p.workgroup, p.staged, p.plane_bytes) == (total, 1024, staged, gw * gh)
        assert p.lds_bytes == base + staged * rows <= MI355X_LDS
        assert m.lanes_preview(params) == {"lds_bytes": total, "workgroup": 1024, "staged": staged, "plane_bytes": gw * gh}
    assert 135952 + 32400 == 168352 > MI355X_LDS             # why 4K without a margin reads its plane from memory
    assert 2 * 39232 <= MI355X_LDS < 2 * 153568              # staged 1080p: still two workgroups per CU
    # rows that are no multiple of 16 bytes are padded; a margin that leaves no row still sizes one
    for (w, h, kw), (gw, R) in [((1040, 144, dict(vertical_mask=0.0)), (65, 9)), ((48, 48, dict(vertical_mask=0.0)), (3, 3)),
                                ((1920, 1080, dict(vertical_mask=0.5)), (120, 1))]:
        params = m.ScanParams.from_config(w, h, **kw)
        rc, p, msg = preview(params)
        assert rc == _abi.MT_OK and p.staged == 1 and p.lds_bytes == dir_lds_by_hand(gw, R) + rows_by_hand(gw, R), msg
    assert rows_by_hand(65, 9) == 592 and rows_by_hand(3, 3) == 16
    # a device with less LDS: staged where the rows fit, unstaged where only the direction scan does, else unsupported
    p1080 = m.ScanParams.from_config(1920, 1080, **config.CODE_DEFAULTS)
    assert preview(p1080, 39232)[1].staged == 1 and preview(p1080, 39231)[1].staged == 0 and preview(p1080, 39231)[1].lds_bytes == 31792
    rc, _, msg = preview(p1080, 31791)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg
    # the grids the plain scan cuts into row bands have no form
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    with pytest.raises(m.MtgpuError) as ei:
        m.lanes_preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(ei.value)
    # invalid
    lib = m.load_library()
    c = p1080.to_c()
    assert lib.mtgpu_lanes_preview(None, MI355X_LDS, C.byref(_abi.LanesPlanC())) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_lanes_preview(C.byref(c), MI355X_LDS, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_lanes_preview(C.byref(c), 100, C.byref(_abi.LanesPlanC())) == _abi.MT_ERR_INVALID


# ------------------------------------------------------------------ error paths that need no device

def test_invalid_arguments_are_rejected_without_a_device():
    """Everything the arguments alone decide is answered before the context is looked at: no HIP call, no byte written."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(64)          # never dereferenced
    odd = C.c_void_p(68)

    def err():
        return lib.mtgpu_last_error().decode()

    def dev(rec=one, rb=40, nrec=1, off=one, n=1, soff=None, ns=0, pl=one, fl=one, ce=one, ro=one):
        return lib.mtgpu_scan_lanes_device(None, rec, rb, nrec, off, None, n, soff, ns, pl, fl, ce, ro, None)

    assert dev(pl=None) == inv and "d_planes is NULL" in err()
    assert dev(pl=None, soff=one, ns=2) == inv and "d_planes is NULL" in err()
    for rb in (0, 7, 16, 39, 41, -8):
        assert dev(rb=rb) == inv and "rec_bytes" in err()
    assert dev(fl=None, ce=None, ro=None) == inv and "all NULL" in err()
    assert dev(off=None) == inv and "d_frame_off" in err()
    assert dev(soff=one) == inv and "d_stream_off is given" in err() and "n_streams is 0" in err()
    assert dev(ns=2) == inv and "n_streams is 2" in err() and "d_stream_off is NULL" in err()
    assert dev(off=odd) == inv and "d_frame_off" in err() and "aligned" in err()
    assert dev(soff=odd, ns=1) == inv and "d_stream_off" in err() and "aligned" in err()
    assert dev(rec=None) == inv and "d_rec" in err()
    assert dev(rec=odd, rb=8) == inv and "d_rec" in err() and "8-byte" in err()
    assert dev(rec=C.c_void_p(66)) == inv and "d_rec" in err()
    assert dev(ce=C.c_void_p(66)) == inv and "d_centres" in err()
    assert dev(ro=C.c_void_p(66)) == inv and "d_rose" in err()
    assert dev(pl=C.c_void_p(67)) == inv and "ctx" in err()             # a plane has no alignment
    assert dev() == inv and "ctx" in err()
    assert dev(soff=one, ns=1) == inv and "ctx" in err()

    def fdev(rec=one, rb=40, nrec=1, off=one, n=1, soff=one, ns=1, flow=one):
        return lib.mtgpu_flow_map_device(None, rec, rb, nrec, off, None, n, soff, ns, flow, None)

    assert fdev(flow=None) == inv and "d_flow is NULL" in err()
    assert fdev(rb=12) == inv and "rec_bytes" in err()
    assert fdev(soff=None) == inv and "d_stream_off is NULL" in err()
    assert fdev(off=None) == inv and "d_frame_off" in err()
    assert fdev(off=odd) == inv and "d_frame_off" in err() and "aligned" in err()
    assert fdev(soff=odd) == inv and "d_stream_off" in err() and "aligned" in err()
    assert fdev(rec=None) == inv and "d_rec" in err()
    assert fdev(rec=odd, rb=8) == inv and "d_rec" in err() and "8-byte" in err()
    assert fdev(flow=C.c_void_p(66)) == inv and "d_flow" in err() and "aligned" in err()
    assert fdev() == inv and "ctx" in err()
    assert fdev(ns=0) == inv and "ctx" in err()

    rose = np.full((2, 8), 7, dtype=np.uint32)
    out = np.full(3, 7, dtype=np.uint32)
    fl = np.full(3, 7, dtype=np.uint8)
    flow = np.full(64, 7, dtype=np.uint32)
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    pl = np.zeros(64, dtype=np.uint8)
    good_off, good_soff = np.array([0, 4, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)

    def host(off=good_off, soff=None, ns=0, planes=pl, f=fl, c=out, r=rose, recs=mv):
        return lib.mtgpu_scan_frames_lanes(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(planes), vp(f), vp(c), vp(r))

    assert host(planes=None) == inv and "planes is NULL" in err()
    assert host(f=None, c=None, r=None) == inv and "all NULL" in err()
    assert host(off=None) == inv and "frame_off" in err()
    assert host(soff=good_soff) == inv and "stream_off is given" in err()
    assert host(ns=1) == inv and "stream_off is NULL" in err()
    assert host(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert host(soff=np.array([0, 2, 1], dtype=np.uint64), ns=2) == inv and "stream_off not monotonic" in err()
    assert host(soff=np.array([0, 1], dtype=np.uint64), ns=1) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(recs=None) == inv and "mv is NULL" in err()
    assert host() == inv and "ctx" in err()
    assert host(soff=good_soff, ns=1) == inv and "ctx" in err()

    def fhost(off=good_off, soff=good_soff, ns=1, fw=flow, recs=mv):
        return lib.mtgpu_flow_map(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(fw))

    assert fhost(fw=None) == inv and "flow is NULL" in err()
    assert fhost(soff=None) == inv and "stream_off is NULL" in err()
    assert fhost(off=None) == inv and "frame_off" in err()
    assert fhost(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert fhost(soff=np.array([0, 1], dtype=np.uint64)) == inv and "stream_off[1]" in err()
    assert fhost(recs=None) == inv and "mv is NULL" in err()
    assert fhost() == inv and "ctx" in err()
    assert out.tolist() == [7, 7, 7] and fl.tolist() == [7, 7, 7] and (rose == 7).all() and (flow == 7).all()


# ------------------------------------------------------------------ lanes.py: planes

def test_plane_from_rects_on_hand_cases():
    # cells: the upper half may not go east, the lower half may do anything; a later rectangle lies over an earlier one
    pl = lanes.plane_from_rects(12, 8, [((0, 0, 12, 4), "S,SW,W,NW,N"), ((3, 2, 5, 6), "E")])
    assert pl.dtype == np.uint8 and pl.shape == (8, 12)
    want = np.full((8, 12), 0xFF, dtype=np.uint8)
    want[0:4, :] = 0x7C
    want[2:6, 3:5] = 0x01
    assert np.array_equal(pl, want)
    assert np.array_equal(lanes.plane_from_rects(12, 8, [], elsewhere=0), np.zeros((8, 12), dtype=np.uint8))
    # pixels: a rectangle covers every cell its 16-pixel blocks intersect; an empty one covers nothing; clipped to the grid
    pl = lanes.plane_from_rects(12, 8, [((15, 16, 33, 17), "W"), ((40, 40, 40, 90), "N"), ((170, 100, 999, 999), 0x03)], elsewhere=0x80,
                                unit="px", shift=4)
    want = np.full((8, 12), 0x80, dtype=np.uint8)
    want[1, 0:3] = 0x10
    want[6:8, 10:12] = 0x03
    assert np.array_equal(pl, want)
    # fractions of the picture
    pl = lanes.plane_from_rects(12, 8, [((0.0, 0.5, 1.0, 1.0), "all"), ((0.0, 0.0, 0.25, 0.5), "none")], elsewhere=0x01, unit="frac",
                                shift=4, size=(192, 128))
    want = np.full((8, 12), 0x01, dtype=np.uint8)
    want[4:8, :] = 0xFF
    want[0:4, 0:3] = 0
    assert np.array_equal(pl, want)
    for bad in ([((0, 0, 1, 1), "X")], [((0, 0, 1, 1), 256)]):
        with pytest.raises(ValueError):
            lanes.plane_from_rects(12, 8, bad)
    with pytest.raises(ValueError):
        lanes.plane_from_rects(12, 8, [], elsewhere=256)


def test_plane_from_flow_and_invert_on_hand_cases():
    flow = np.zeros((8, 2, 3), dtype=np.uint32)
    flow[:, 0, 0] = [100, 0, 0, 0, 0, 0, 0, 0]        # everything goes east
    flow[:, 0, 1] = [60, 0, 0, 0, 40, 0, 0, 0]        # a two-way cell
    flow[:, 0, 2] = [3, 0, 0, 0, 0, 0, 0, 0]          # too few records
    flow[:, 1, 0] = [0, 0, 0, 63, 0, 0, 193, 0]       # 63 * 256 = 16128 < 64 * 256 = 16384: SW stays out at a quarter
    flow[:, 1, 1] = [0, 0, 0, 64, 0, 0, 192, 0]       # 64 * 256 = 16384 >= 16384: SW is in
    flow[:, 1, 2] = [2, 2, 2, 2, 2, 2, 2, 2]          # every sector holds an eighth
    pl = lanes.plane_from_flow(flow, min_records=16, share_q8=64, widen=0, elsewhere=0xFF)
    assert pl.tolist() == [[0x01, 0x11, 0xFF], [0x40, 0x48, 0x00]]
    pl1 = lanes.plane_from_flow(flow, min_records=16, share_q8=64, widen=1, elsewhere=0xFF)
    assert pl1.tolist() == [[0x83, 0xBB, 0xFF], [0xE0, 0xFC, 0x00]]          # each usual sector and its two neighbours
    assert lanes.plane_from_flow(flow, min_records=16, share_q8=32, widen=0, elsewhere=0x55).tolist() == [[0x01, 0x11, 0x55], [0x48, 0x48, 0xFF]]
    assert lanes.plane_from_flow(flow, min_records=2, share_q8=64, widen=0, elsewhere=0)[0, 2] == 0x01
    assert lanes.plane_from_flow(flow, min_records=16, share_q8=64, widen=4, elsewhere=0)[0, 0] == 0xFF
    learned = lanes.learned_from_flow(flow, 16)
    assert learned.tolist() == [[True, True, False], [True, True, True]]
    assert lanes.invert_plane(pl1, learned, elsewhere=0).tolist() == [[0x7C, 0x44, 0x00], [0x1F, 0x03, 0xFF]]
    assert lanes.invert_plane(pl1, learned, elsewhere=0xFF)[0, 2] == 0xFF
    assert lanes.dominant_sector(flow, 16).tolist() == [[0, 0, -1], [6, 6, 0]]
    assert lanes.glyph_rows(lanes.dominant_sector(flow, 16), ascii_only=True) == ["00.", "660"]
    assert lanes.glyph_rows(lanes.dominant_sector(flow, 16)) == ["→→·", "↑↑→"]
    # a plane and its inverse never both let a sector vote in a learned cell, and between them they let every sector vote
    inv = lanes.invert_plane(pl1, learned, 0)
    assert ((pl1 & inv)[learned] == 0).all() and ((pl1 | inv)[learned] == 0xFF).all()
    for bad in (dict(share_q8=257), dict(share_q8=-1), dict(widen=5), dict(widen=-1), dict(elsewhere=256)):
        with pytest.raises(ValueError):
            lanes.plane_from_flow(flow, **dict(dict(min_records=1, share_q8=64, widen=0, elsewhere=0), **bad))
    with pytest.raises(ValueError):
        lanes.plane_from_flow(np.zeros((7, 2, 3), dtype=np.uint32))
    with pytest.raises(ValueError):
        lanes.invert_plane(pl1, learned[:1], 0)


def test_mtdir_round_trip_and_malformed_files(tmp_path):
    rng = np.random.RandomState(11)
    for gw, gh in ((1, 1), (12, 8), (65, 9), (240, 135)):
        plane = rng.randint(0, 256, size=(gh, gw)).astype(np.uint8)
        path = str(tmp_path / f"p{gw}x{gh}.mtdir")
        lanes.save_plane(path, plane)
        text = open(path).read().split("\n")
        assert text[0] == "mtdir 1" and text[1] == f"{gw} {gh}" and len(text) == gh + 3 and all(len(t) == 2 * gw for t in text[2:-1])
        got = lanes.load_plane(path)
        assert got.dtype == np.uint8 and np.array_equal(got, plane)
        assert np.array_equal(lanes.load_plane(path, grid=(gw, gh)), plane)
    good = "mtdir 1\n3 2\n01ff10\nAb00Cd\n"
    path = str(tmp_path / "hand.mtdir")
    open(path, "w").write(good)
    assert lanes.load_plane(path).tolist() == [[0x01, 0xFF, 0x10], [0xAB, 0x00, 0xCD]]
    open(path, "w").write(good.replace("\n", "\r\n"))
    assert lanes.load_plane(path).tolist() == [[0x01, 0xFF, 0x10], [0xAB, 0x00, 0xCD]]
    with pytest.raises(ValueError, match="line 2.*3x2.*4x2"):
        lanes.load_plane(path, grid=(4, 2))
    for text, line in (("mtkeep 1\n3 2\n01ff10\nab00cd\n", 1), ("", 1), ("mtdir 1\n", 2), ("mtdir 1\n3\n", 2), ("mtdir 1\n3 0\n", 2),
                       ("mtdir 1\n3 x\n", 2), ("mtdir 1\n3 2\n01ff10\n", 4), ("mtdir 1\n3 2\n01ff1\nab00cd\n", 3),
                       ("mtdir 1\n3 2\n01ff10\nab00cd00\n", 4), ("mtdir 1\n3 2\n01ff10\nab0gcd\n", 4), ("mtdir 1\n3 2\n01 f10\nab00cd\n", 3),
                       ("mtdir 1\n3 2\n01ff10\nab00cd\n00\n", 5)):
        open(path, "w").write(text)
        with pytest.raises(ValueError, match=f"line {line}:"):
            lanes.load_plane(path)
    for bad in (np.zeros((2, 3), dtype=np.int32), np.zeros(3, dtype=np.uint8), np.zeros((0, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            lanes.save_plane(path, bad)


def test_lanes_options_parse():
    a = lanes.parser().parse_args(["f.mtmv", "--learn", "--min-records", "8", "--share", "0.5", "--widen", "2", "--save-plane", "p.mtdir"])
    assert a.learn and (a.min_records, a.share, a.widen, a.save_plane) == (8, 0.5, 2, "p.mtdir")
    a = lanes.parser().parse_args(["f", "--lane", "0,0,960,540:W,NW,SW", "--lane", "0,540,1920,1080:all", "--elsewhere", "none", "--json"])
    assert a.lane == [((0.0, 0.0, 960.0, 540.0), 0x38), ((0.0, 540.0, 1920.0, 1080.0), 0xFF)] and a.elsewhere == "none" and a.json
    a = lanes.parser().parse_args(["f", "--plane", "p.mtdir", "--invert"])
    assert a.plane == "p.mtdir" and a.invert and a.elsewhere is None and not a.learn


@pytest.mark.parametrize("bad", [[], ["--learn", "--plane", "p"], ["--learn", "--invert"], ["--plane", "p", "--lane", "0,0,1,1:E"],
                                 ["--plane", "p", "--save-plane", "q"], ["--lane", "0,0,1:E"], ["--lane", "0,0,1,1"], ["--lane", "0,0,1,1:X"],
                                 ["--lane", "5,0,1,1:E"], ["--lane", "0,0,1.5,1:E"], ["--learn", "--share", "1.5"], ["--learn", "--widen", "5"],
                                 ["--learn", "--min-records", "-1"], ["--plane", "p", "--elsewhere", "some"]])
def test_lanes_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch):
    """argparse's exit code 2, and neither the file nor a scanner has been looked at."""
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(lanes, "MotionScanner", boom)
    monkeypatch.setattr(lanes.tune, "load", boom)
    monkeypatch.setattr(lanes.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        lanes.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2


def test_lanes_missing_files_exit_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the files were read")
    monkeypatch.setattr(lanes, "MotionScanner", boom)
    assert lanes.main([str(tmp_path / "nothing_here.json"), "--learn"]) == 1
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.mtmv")
    m.mvfile.write_mtmv(path, 160, 160, 1, 1000, 25.0, 1.0, [0], [mv])
    assert lanes.main([path, "--plane", str(tmp_path / "nothing_here.mtdir")]) == 1
    bad = str(tmp_path / "bad.mtdir")
    open(bad, "w").write("mtdir 1\n10 10\n")
    assert lanes.main([path, "--plane", bad]) == 1
    lanes.save_plane(bad, np.zeros((3, 3), dtype=np.uint8))
    with pytest.raises(SystemExit) as ei:                   # a plane of another grid
        lanes.main([path, "--plane", bad])
    assert ei.value.code == 2


# ------------------------------------------------------------------ the model, the oracle and the hand values

def check_case(c, planes=None, soff="case"):
    """The model equals the oracle on filtered records (consequence C); returns the model's (flags, centres, rose)."""
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    planes = c["planes"] if planes is None else planes
    soff = c["soff"] if isinstance(soff, str) else soff
    fl, ce, rose = lm.model_batch(p, mv, off, sd, planes, soff)
    ofl, oce = lm.oracle_batch(p, mv, off, sd, planes, soff)
    assert ce.tolist() == oce.tolist() and fl.tolist() == ofl.tolist()
    # the rose is the direction scan's, whatever the planes hold
    owned = lm.frame_planes(len(off) - 1, planes, soff) >= 0
    assert rose.sum(axis=1).tolist() == np.where(owned, dm.counting_moving(p, mv, off, sd), 0).tolist()
    return fl, ce, rose


def check_flow(c, soff=None):
    """Consequence G on the model: per stream and sector the flow map sums to the roses of the stream's frames."""
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    F = len(off) - 1
    soff = (c["soff"] if c["soff"] is not None else np.array([0, F], dtype=np.uint64)) if soff is None else soff
    flow = lm.flow_map(p, mv, off, sd, soff)
    rose = dm.model_batch(p, mv, off, sd, allow=0xFF)[2]
    for s in range(len(soff) - 1):
        a, b = int(soff[s]), int(soff[s + 1])
        assert flow[s].sum(axis=(1, 2)).tolist() == rose[a:b].sum(axis=0).tolist()
    mg = p.vertical_margin
    assert not flow[:, :, :mg].any() and not flow[:, :, p.grid_h - mg:].any() if mg else True
    return flow


@pytest.mark.parametrize("name", sorted(li.HAND_CASES))
def test_hand_frames(name):
    c = li.HAND_CASES[name]()
    fl, ce, rose = check_case(c)
    assert ce.tolist() == c["hand_centres"].tolist() and rose.tolist() == c["hand_rose"].tolist()
    # the one-plane form gives each stream's values when it is handed that stream's plane
    for s in range(len(c["planes"])):
        a, b = int(c["soff"][s]), int(c["soff"][s + 1])
        _, ce1, rose1 = lm.model_batch(c["params"], c["mv"], c["off"], c["sd"], c["planes"][s])
        assert ce1[a:b].tolist() == ce[a:b].tolist() and rose1[a:b].tolist() == rose[a:b].tolist()
    check_flow(c)


def test_hand_flow_map():
    c = li.one_cell_case()
    flow = check_flow(c)
    want = np.zeros((3, 8, 5, 6), dtype=np.uint32)
    want[:, 0, 1, 2], want[:, 4, 1, 2], want[:, 0, 1, 3] = 1, 1, 2
    assert np.array_equal(flow, want)
    # the margin rows and the still records count nowhere
    flow = check_flow(li.margin_case())
    assert flow[0, 0].sum() == 4 and flow[0, 0, 1, 2] == 1 and flow[0, 0, 0, 2] == 0 and flow[0, 0, 7, 4] == 0
    flow = check_flow(li.still_case())
    assert flow.sum() == 2 and flow[0, 0, 1, 3] == 1


def test_uniform_planes_are_the_direction_scan():
    """Consequences A and B on the model: a plane filled with one byte is that allow byte; 0xFF is the plain scan."""
    import dir_inputs as di
    c = di.edge_case()
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    for byte in (di.EDGE_ALLOW, 0xFF):
        want = dm.model_batch(p, mv, off, sd, allow=byte)
        got = lm.model_batch(p, mv, off, sd, np.full((p.grid_h, p.grid_w), byte, dtype=np.uint8))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    plain = ob.scan_centres(p, mv, off, sd, nthreads=4)
    assert got[1].tolist() == plain[1].tolist() and got[0].tolist() == plain[0].tolist()
    c = di.boundary_case()
    p = c["params"]
    planes = np.stack([np.full((p.grid_h, p.grid_w), a, dtype=np.uint8) for a in c["allows"]])
    got = lm.model_batch(p, c["mv"], c["off"], c["sd"], planes, c["soff"])
    assert got[1].tolist() == di.BOUNDARY_HAND and got[2].tolist() == [di.BOUNDARY_ROSE] * len(di.BOUNDARY_HAND)


@pytest.mark.parametrize("gw", [65, 129])
def test_word_seam_hand_values(gw):
    c = li.seam_case(gw)
    fl, ce, rose = check_case(c)
    assert ce.tolist() == c["hand_centres"].tolist() == li.SEAM_HAND[gw] and rose.tolist() == c["hand_rose"].tolist()
    assert (c["params"].grid_w + 63) // 64 == (2 if gw == 65 else 3)
    pl = c["planes"]
    assert (pl[0, :, 63] != pl[0, :, 64]).all() and (pl[1, :, 63] != pl[1, :, 64]).all() and pl[0].size % 2 == 1
    if gw == 129:
        assert (pl[0, :, 127] != pl[0, :, 128]).all()
    check_flow(c)


def test_uhd_input_has_both_forms():
    for mask, staged in ((0.0, 0), (0.05, 1)):
        c = li.uhd_case(mask)
        assert m.lanes_preview(c["params"])["staged"] == staged
        fl, ce, rose = check_case(c)
        full = lm.model_batch(c["params"], c["mv"], c["off"], c["sd"], np.full_like(c["planes"], 0xFF))[1]
        lengths = np.diff(c["off"].astype(np.int64))
        assert 200 <= lengths.min() and lengths.max() <= 1200 and (ce > 0).all() and (ce < full).all()
        assert len(np.unique(c["planes"])) == 256
    # the two forms see the same plane and the same records; the margin rows of the staged one hold records that do not count
    a, b = li.uhd_case(0.0), li.uhd_case(0.05)
    assert np.array_equal(a["planes"], b["planes"]) and a["mv"].tobytes() == b["mv"].tobytes()
    assert lm.model_batch(b["params"], b["mv"], b["off"], b["sd"], b["planes"])[2].sum() < \
        lm.model_batch(a["params"], a["mv"], a["off"], a["sd"], a["planes"])[2].sum()


def test_three_piece_input():
    c = li.pieces_case()
    fl, ce, rose = check_case(c)
    assert ce.tolist() == [3, 6] == c["hand_centres"].tolist() and rose.tolist() == c["hand_rose"].tolist()
    assert li.PIECES_N > 2 * 128 * 1024 and len(c["mv"]) == 2 * li.PIECES_N
    column = c["planes"][0][:, li.PIECES_COLUMN]
    assert ((column >> li.PIECES_SECTOR) & 1).tolist() == [0, 0, 0, 1, 1, 1]


def test_stream_input():
    import dir_inputs as di
    c = li.stream_case()
    fl, ce, rose = check_case(c)
    F = len(c["sd"])
    assert np.diff(c["soff"].astype(np.int64)).tolist() == di.STREAM_SIZES and len(c["planes"]) == 7
    orphan = np.r_[0:3, F - 5:F]
    assert not ce[orphan].any() and not rose[orphan].any() and (np.diff(c["off"].astype(np.int64))[orphan] > 0).all()
    k = di.STREAM_KEY_FRAME
    assert c["sd"][k] == 0 and ce[k] == 0 and not rose[k].any()
    # the planes differ: one plane for every frame gives other counts, and reaches the orphans
    one = check_case(c, c["planes"][6], None)[1]
    assert (one != ce).sum() > 20 and (ce > 0).sum() > 30 and 0 < fl.sum() < F and one[orphan].any()
    flow = check_flow(c)
    assert not flow[0].any() and not flow[4].any() and flow[3].any() and flow[6].any()


@pytest.mark.parametrize("i", range(li.N_DRAWS))
def test_random_draws_have_the_consequences(i):
    """C (inside check_case), D along the chain, E against the oracle's masked count, F, G on draw i — all on the model."""
    c = li.draw(i)
    p, mv, off, sd = c["params"], c["mv"], c["off"], c["sd"]
    plain_f, plain_c = ob.scan_centres(p, mv, off, sd, nthreads=4)
    prev = None
    for plane in c["chain"]:
        fl, ce, rose = check_case(c, plane, None)
        if prev is not None:
            assert (prev <= ce).all()                                                      # D
        prev = ce
        if p.vectors_needed == 0:
            assert ce.tolist() == plain_c.tolist()                                         # F
    assert prev.tolist() == plain_c.tolist() and fl.tolist() == plain_f.tolist()           # B
    if p.vectors_needed >= 1 and p.mv_threshold_sq >= 1.0:                                 # E
        ze = check_case(c, c["zones"], None)[1]
        want = zi.model_batch(p, mv, off, sd, np.array([0, len(sd)], dtype=np.uint64), lm.zones_keep(c["zones"])[None])[0]
        assert ze.tolist() == want.tolist()
    if i < li.N_FLOW_DRAWS:
        check_flow(c)                                                                      # G
