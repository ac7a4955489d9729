"""CPU tier: object headings (include/mtgpu_headings.h) exist at every layer — header, library, ctypes table, Python
module, command, example — size their launch with host arithmetic alone and reject bad arguments before any HIP call;
the numpy restatement (tests/headings_model.py) returns every hand number of tests/headings_inputs.py and holds
consequences D and E against the unchanged oracle and dir_model; the new kernel unit compiles to three kernels without
scratch, without a spilled register, at eight waves per SIMD."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, direction, headings, objects

import blobs_inputs as bi
import dir_model as dm
import headings_inputs as hi
import headings_model as hm
import objects_inputs as oi
import oracle_binding as ob
from test_derived_kernel_resources_host import compile_unit
from test_scan_kernel_resources_host import CSRC, makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_headings_preview", "mtgpu_scan_frames_headings", "mtgpu_scan_headings_device"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_headings.h")).read()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_HEADINGS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_HEADINGS[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        at = hdr.index("int " + n + "(")          # every declaration names the reference lines it stands for
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert _abi.ABI_HEADINGS in _abi.ABI_TABLES
    assert C.sizeof(_abi.HeadingsPlanC) == 16
    assert [f for f, _ in _abi.HeadingsPlanC._fields_] == ["lds_bytes", "workgroup", "keep_words_per_row", "keep_words_per_stream"]
    dt = _abi.HEADING_DTYPE
    assert dt.itemsize == 64 and dt.names == ("n", "records", "heading", "sum_dx", "sum_dy", "reserved")
    assert [dt.fields[n][1] for n in dt.names] == [0, 32, 36, 40, 48, 56] and dt["n"].shape == (8,)
    assert [dt[n].base for n in dt.names] == [np.dtype(t) for t in ("<u4", "<u4", "<u4", "<i8", "<i8", "<u8")]
    assert (_abi.HEADING_NONE, _abi.HEADING_TABLE_BYTES) == (0xFFFFFFFF, 56) == (hm.NONE, hi.TABLE_BYTES)
    assert "#define MT_HEADING_NONE 0xFFFFFFFFu" in hdr and "#define MT_HEADING_TABLE_BYTES 56" in hdr
    top = open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert top.count('#include "mtgpu_headings.h"') == 1 and not any(n in top for n in NEW_SYMBOLS)
    # the header states the consequences the GPU tests rest on, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("centres, blobs, objects and list are mtgpu_scan_objects_device's, bit for bit", "allowed[f] == min(objects[f], k)",
                 "flags are the object scan's flags bit for bit", "motion does not depend on allow, min_blob_cells or min_objects",
                 "motion for k is the first k entries per frame of motion for MT_OBJECTS_MAX", "sum(n) <= records",
                 "records >= cells vectors_needed", "at most rose[f].n[s] of mtgpu_scan_dir_device", "n'[(s + 2) & 7] = n[s]",
                 "sum_dx' = -sum_dy, sum_dy' = sum_dx", "heading' = (heading + 2) & 7", "allowed <= allowed'",
                 "A still object has no direction to object to", "the LOWEST such sector on a tie", "Out of scope: per-stream allow bytes",
                 "a compensated form", "the C++ host layer and mtgpu_scan_file", "velocity prediction", "row-banded grids"):
        assert text in flat, text
    # the sentence the object header keeps
    assert "no per-object direction" in open(os.path.join(ROOT, "include", "mtgpu_objects.h")).read()
    src = open(os.path.join(CSRC, "headings_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "objects_frames_kernel<" not in src
    for inc in ('"record_stream.h"', '"blob_label.h"', '"blob_rank.h"'):
        assert "#include " + inc in src, inc
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "headings_kernels.hip" in mk and "headings_kernels.h " in mk and "mtgpu_headings.h" in mk
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"headings_frames_kernel" in blob and b"headings_clear_kernel" in blob


def test_headers_compile_as_c_and_cpp_in_any_order(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_headings_plan p;\n"
            "  mt_heading h = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, MT_HEADING_NONE, 0, 0, 0};\n"
            "  mt_object o = {0, 0, 0, 0, 0, 0};\n"
            "  mt_dir_rose r;\n"
            "  return mtgpu_headings_preview(0, MT_OBJECTS_MAX, 163840, &p)\n"
            "       + mtgpu_scan_headings_device(c, 0, 40, 0, 0, 0, 0, 0, 0, 0, 4, 1, 1, 255, 0, 0, 0, 0, &o, &h, 0, 0)\n"
            "       + mtgpu_scan_frames_headings(c, 0, 0, 0, 0, 0, 0, 0, 4, 1, 1, 255, 0, 0, 0, 0, &o, &h, 0)\n"
            "       + p.lds_bytes + p.workgroup + p.keep_words_per_row + p.keep_words_per_stream + (int)(h.n[7] + h.records + h.heading)\n"
            "       + (int)(h.sum_dx + h.sum_dy) + (int)h.reserved + (int)sizeof r + MT_HEADING_TABLE_BYTES;\n}\n"
            "typedef char heading_is_64_bytes[sizeof(mt_heading) == 64 ? 1 : -1];\n")
    orders = [("mtgpu.h",), ("mtgpu_headings.h",), ("mtgpu_headings.h", "mtgpu_objects.h", "mtgpu_dir.h"),
              ("mtgpu_objects.h", "mtgpu_headings.h", "mtgpu_dir.h"), ("mtgpu_dir.h", "mtgpu_objects.h", "mtgpu_headings.h"),
              ("mtgpu_dir.h", "mtgpu_headings.h", "mtgpu_objects.h")]
    for i, order in enumerate(orders):
        src = tmp_path / f"use_{i}.c"
        src.write_text("".join('#include "%s"\n' % h for h in order) + body)
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang, "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/headings_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "headings_example.c")])


def test_canary_program_builds(tmp_path):
    """The plain-C contract program of the GPU tier compiles and links against the ABI (it cannot run without a device);
    its struct checks — 64 bytes, the offsets of the header — are compile-time."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_headings_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_headings_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_package_exports_the_module_not_methods():
    """The Python layer lives in mvtrim_amd.headings: MotionScanner's methods and the package's export list are a recorded
    surface (tests/golden/scanner_calls.json) and stay what they were."""
    assert headings.HEADING_DTYPE is _abi.HEADING_DTYPE and headings.NO_HEADING == 0xFFFFFFFF
    assert headings.OUTPUTS == objects.OUTPUTS + ("motion", "allowed")
    assert not hasattr(m.MotionScanner, "scan_headings") and "headings" not in m.__all__
    for name in ("preview", "scan", "scan_device", "mean_vector", "main", "measure", "parser", "heading_histogram"):
        assert callable(getattr(headings, name)), name
    mo = hi.motion_of([([4, 0, 0, 0, 0, 0, 0, 0], 4, 0, 31, 6), ([0] * 8, 2, hm.NONE, 0, 0)], 3)
    assert headings.mean_vector(mo).tolist() == [[7.75, 1.5], [0.0, 0.0], [0.0, 0.0]]
    cells, head = np.array([[3, 3, 2, 0]]), np.array([[0, 4, hm.NONE, hm.NONE]])
    assert headings.heading_histogram(cells, head, 1) == {"E": 1, "SE": 0, "S": 0, "SW": 0, "W": 1, "NW": 0, "N": 0, "NE": 0, "none": 1}
    assert headings.heading_histogram(cells, head, 3)["none"] == 0


# ------------------------------------------------------------------ the kernel unit

@pytest.fixture(scope="module")
def unit_resources(tmp_path_factory):
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    assert os.path.exists(os.path.join(CSRC, "headings_kernels.hip"))
    return compile_unit(("headings", hipcc, flags, str(tmp_path_factory.mktemp("headings_res") / "headings_kernels.o")))[1]


def test_the_unit_holds_three_kernels_without_scratch_at_eight_waves(unit_resources):
    """Three kernels: the 40-byte and the 8-byte form of headings_frames_kernel and headings_clear_kernel.  No scratch, no
    spilled register, eight waves per SIMD: two 1080p workgroups per CU need it."""
    for n, r in sorted(unit_resources.items()):
        print(n, r)
    frames = sorted(n for n in unit_resources if "headings_frames_kernel" in n)
    clear = [n for n in unit_resources if "headings_clear_kernel" in n]
    assert len(frames) == 2 and len(clear) == 1 and len(unit_resources) == 3, sorted(unit_resources)
    assert [bool(re.search(r"headings_frames_kernelILi1024ELi\d+ELi%dEE" % rec, n)) for n, rec in zip(frames, (40, 8))] == [True, True], frames
    assert not any("objects_frames_kernel" in n for n in unit_resources)
    for n in frames + clear:
        r = unit_resources[n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["Occupancy"] >= 8, (n, r)


# ------------------------------------------------------------------ preview

def preview(params, k, lds=MI355X_LDS):
    p = _abi.HeadingsPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_headings_preview(C.byref(c), k, lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def test_preview_is_the_object_layout_plus_the_table():
    for w, h, kw in [(1920, 1080, {}), (3840, 2160, {}), (3840, 2160, dict(vertical_mask=0.0)), (1280, 720, {}),
                     (48, 48, dict(vertical_mask=0.0)), (1920, 1080, dict(vertical_mask=0.5))]:
        params = m.ScanParams.from_config(w, h, **kw)
        R = max(1, params.grid_h - 2 * params.vertical_margin)
        for k in (1, 16):
            obj = objects.preview(params, k)
            rc, p, msg = preview(params, k)
            assert rc == _abi.MT_OK, msg
            assert p.lds_bytes == obj["lds_bytes"] + k * 56 == hi.lds_by_hand(params.grid_w, R, k) <= MI355X_LDS
            assert (p.workgroup, p.keep_words_per_row, p.keep_words_per_stream) == (1024, obj["keep_words_per_row"], obj["keep_words_per_stream"])
            assert headings.preview(params, k) == {"lds_bytes": p.lds_bytes, "workgroup": 1024, "keep_words_per_row": p.keep_words_per_row,
                                                   "keep_words_per_stream": p.keep_words_per_stream}
    # 1080p at k = 16 with every row analysed: the figure of the design, and two workgroups share a CU's LDS
    assert headings.preview(m.ScanParams.from_config(1920, 1080, vertical_mask=0.0), 16)["lds_bytes"] == 37120 and 2 * 37120 <= MI355X_LDS


def test_preview_refusals():
    lib = m.load_library()
    good = m.ScanParams.from_config(1920, 1080)
    c = good.to_c()
    inv = _abi.MT_ERR_INVALID
    for k in (0, -1, 17, 1 << 20):
        rc, _, msg = preview(good, k)
        assert rc == inv and "k is %d" % k in msg, (k, msg)
    assert lib.mtgpu_headings_preview(None, 4, MI355X_LDS, C.byref(_abi.HeadingsPlanC())) == inv
    assert lib.mtgpu_headings_preview(C.byref(c), 4, MI355X_LDS, None) == inv
    assert lib.mtgpu_headings_preview(C.byref(c), 4, 100, C.byref(_abi.HeadingsPlanC())) == inv
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2), 1)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0), 16)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    rc, _, msg = preview(good, 16, 16384)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg and "16 objects" in msg
    with pytest.raises(m.MtgpuError) as ei:
        headings.preview(good, 17)
    assert ei.value.code == inv


@pytest.mark.parametrize("k", [1, 2, 8, 15, 16])
def test_the_last_grid_each_k_accepts(k):
    """By bisection over the preview (the input of the GPU tier's cliff case): the tallest 65-column grid for k entries
    fits by the hand formula, one more row does not and is refused with the grid named; it is never taller than the
    object scan's."""
    gh = hi.cliff_rows(k)
    assert hi.lds_by_hand(65, gh, k) <= MI355X_LDS < hi.lds_by_hand(65, gh + 1, k)
    rc, p, msg = preview(bi.limit_params(65, gh), k)
    assert rc == _abi.MT_OK and p.lds_bytes == hi.lds_by_hand(65, gh, k), msg
    rc, _, msg = preview(bi.limit_params(65, gh + 1), k)
    assert rc == _abi.MT_ERR_UNSUPPORTED and f"65x{gh + 1}" in msg, msg
    assert 500 < gh <= oi.cliff_rows(k)


# ------------------------------------------------------------------ error paths that need no device

def test_invalid_arguments_are_rejected_without_a_device():
    """Everything the arguments alone decide is answered before the context is looked at: no HIP call, no byte written."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(64)          # never dereferenced
    odd = C.c_void_p(68)

    def err():
        return lib.mtgpu_last_error().decode()

    def dev(rec=one, rb=40, nrec=1, off=one, n=1, soff=one, ns=1, keep=one, k=4, mo=1, allow=255, fl=one, ce=one, bl=one, ob=one, li=one,
            mot=one, al=one):
        return lib.mtgpu_scan_headings_device(None, rec, rb, nrec, off, None, n, soff, ns, keep, k, 1, mo, allow, fl, ce, bl, ob, li, mot, al, None)

    for k in (0, 17, -3):
        assert dev(k=k) == inv and "k is %d" % k in err()
    assert dev(mo=5) == inv and "min_objects is 5, above k = 4" in err()
    assert dev(k=16, mo=17) == inv and "min_objects is 17" in err()
    for a in (-1, 256, 1 << 20):
        assert dev(allow=a) == inv and "allow %d" % a in err()
    for rb in (0, 7, 16, 39, 41, -8):
        assert dev(rb=rb) == inv and "rec_bytes" in err()
    assert dev(fl=None, ce=None, bl=None, ob=None, li=None, mot=None, al=None) == inv and "all NULL" in err()
    assert dev(off=None) == inv and "d_frame_off" in err()
    assert dev(soff=None) == inv and "d_stream_off" in err()
    assert dev(ns=0) == inv and "n_streams" in err()
    assert dev(keep=None) == inv and "d_keep" in err()
    assert dev(off=odd) == inv and "d_frame_off" in err() and "aligned" in err()
    assert dev(keep=odd) == inv and "d_keep" in err() and "aligned" in err()
    assert dev(rec=None) == inv and "d_rec" in err()
    assert dev(rec=odd, rb=8) == inv and "d_rec" in err() and "8-byte" in err()
    assert dev(al=C.c_void_p(66)) == inv and "d_allowed" in err()
    assert dev(ob=C.c_void_p(66)) == inv and "d_objects" in err()
    for a in (65, 66, 68, 72):
        assert dev(mot=C.c_void_p(a)) == inv and "d_motion must be 16-byte aligned" in err(), a
        assert dev(li=C.c_void_p(a)) == inv and "d_list must be 16-byte aligned" in err(), a
    assert dev() == inv and "ctx" in err()
    assert dev(keep=None, soff=None, ns=0) == inv and "ctx" in err()         # the form without a mask is a valid one
    assert dev(k=16, mo=16) == inv and "ctx" in err() and dev(k=1, mo=0, allow=0) == inv and "ctx" in err()
    assert dev(fl=None, ce=None, bl=None, ob=None, li=None, al=None) == inv and "ctx" in err()      # motion alone

    out = np.full(3, 7, dtype=np.uint32)
    fl = np.full(3, 7, dtype=np.uint8)
    mot = np.full((3, 4, 64), 7, dtype=np.uint8)
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    keep = np.zeros(4, dtype=np.uint64)
    good_off, good_soff = np.array([0, 4, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)

    def host(off=good_off, soff=good_soff, ns=1, kp=keep, k=4, mo=1, allow=255, f=fl, a=out, mt=mot, recs=mv):
        return lib.mtgpu_scan_frames_headings(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(kp), k, 1, mo, allow, vp(f), None, None, None,
                                              None, vp(mt), vp(a))

    assert host(k=0) == inv and "k is 0" in err()
    assert host(mo=5) == inv and "min_objects is 5" in err()
    assert host(allow=256) == inv and "allow 256" in err()
    assert host(f=None, a=None, mt=None) == inv and "all NULL" in err()
    assert host(soff=None) == inv and "stream_off" in err()
    assert host(off=None) == inv and "frame_off" in err()
    assert host(ns=0) == inv and "n_streams" in err()
    assert host(kp=None) == inv and "keep is NULL" in err()
    assert host(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert host(soff=np.array([0, 1], dtype=np.uint64)) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(recs=None) == inv and "mv is NULL" in err()
    assert host() == inv and "ctx" in err()
    assert host(kp=None, soff=None, ns=0) == inv and "ctx" in err()
    assert out.tolist() == [7, 7, 7] and fl.tolist() == [7, 7, 7] and (mot == 7).all()


# ------------------------------------------------------------------ the model

def test_model_returns_every_hand_number():
    """The three blobs by hand at both thresholds, with and without the mask, at k = 1, 2, 3, 16 and every allow byte of
    the table; seventeen blobs; the seams; the frame of 40 000 records."""
    for thr in (16, 0):
        p, mv, off, sd, soff, keeps = hi.hand_case(thr)
        for k in (1, 2, 3, 16):
            for (t, allow, mbc) in hi.HAND_ALLOWED:
                if t != thr:
                    continue
                for masked in (False, True):
                    got = hm.model_batch(p, mv, off, sd, k, mbc, allow, soff if masked else None, keeps if masked else None)
                    want = hi.hand_want(thr, k, mbc, allow, masked)
                    assert sorted(want) == sorted(got)
                    for n in want:
                        assert hm.same(got[n], want[n]), (thr, k, allow, mbc, masked, n)
    p, mv, off, sd = hi.seventeen_case()
    for k in (1, 2, 15, 16):
        got = hm.model_batch(p, mv, off, sd, k)
        assert hm.same(got["motion"], hi.seventeen_motion(k)) and got["blobs"].tolist() == [17], k
    p, mv, off, sd, hand = hi.seams_case()
    got = hm.model_batch(p, mv, off, sd, 16)
    assert hm.same(got["motion"], hi.motion_of(hand, 16)[None]) and hm.same(got["list"], oi.om.entries(oi.SEAM_LIST, 16)[None])
    p, mv, off, sd = hi.big_case()
    got = hm.model_batch(p, mv, off, sd, 2)
    assert got["list"][1, 0].tolist() == hi.BIG_LIST and hm.same(got["motion"][1], hi.motion_of([hi.BIG_MOTION], 2))
    assert int(got["motion"]["sum_dx"][1, 0]) == 40000 * 65535 > 2 ** 31 and got["blobs"].tolist() == [0, 1]


@pytest.mark.parametrize("seed", range(6))
def test_model_holds_d_and_e_against_the_oracle_and_dir_model(seed):
    """On random draws, without a mask: the model's centres are the unchanged oracle's; per sector the entries' bins sum
    to at most dir_model's rose (D); sum(n) <= records and records >= cells * vectors_needed (D); under the quarter turn
    the list stays and motion turns (E)."""
    p, mv, off, sd, _, _ = hi.random_case(seed)
    got = hm.model_batch(p, mv, off, sd, 16)
    _, centres = ob.scan_centres(p, mv, off, sd, nthreads=2)
    assert got["centres"].tolist() == centres.tolist()
    _, _, rose = dm.model_batch(p, mv, off, sd)
    n = got["motion"]["n"].astype(np.int64)
    assert (n.sum(axis=1) <= rose).all()
    rec = got["motion"]["records"].astype(np.int64)
    assert (n.sum(axis=-1) <= rec).all() and (rec >= got["list"]["cells"].astype(np.int64) * p.vectors_needed).all()
    assert int(rec.sum()) > 0
    turned = hm.model_batch(p, hm.quarter_turn(mv), off, sd, 16)
    exp = hm.turned(got["motion"])
    assert hm.same(turned["list"], got["list"])
    for name in ("n", "records", "sum_dx", "sum_dy"):
        assert np.array_equal(turned["motion"][name], exp[name]), name
    u = hm.unique_max(got["motion"])
    assert np.array_equal(turned["motion"]["heading"][u], exp["heading"][u])
    # C and F on the model: the head of the list, and monotone in the allow byte
    for k in (1, 5):
        assert hm.same(hm.model_batch(p, mv, off, sd, k)["motion"], got["motion"][:, :k])
    a = [hm.model_batch(p, mv, off, sd, 16, 1, byte)["allowed"] for byte in (0, 0x11, 0x55, 0xFF)]
    assert all((x <= y).all() for x, y in zip(a, a[1:])) and a[-1].tolist() == np.minimum(got["objects"], 16).tolist()


# ------------------------------------------------------------------ the command

def test_headings_options_parse():
    a = headings.parser().parse_args(["f.mtmv", "--top", "4", "--min-blob-cells", "3", "--min-objects", "1,2,4", "--allow", "E,NE",
                                      "--keep", "cam.mtkeep", "--json", "--width", "1920", "--height", "1080", "--duration", "12.5"])
    assert (a.top, a.min_blob_cells, a.min_objects, a.keep, a.json) == (4, 3, [1, 2, 4], "cam.mtkeep", True)
    assert headings.allow_of(a) == direction.allow_from_names("E,NE") == 0x81
    a = headings.parser().parse_args(["f", "--ignore", "W"])
    assert (a.top, a.min_blob_cells, a.min_objects, a.keep, a.json) == (16, 1, [1, 2, 3], None, False) and headings.allow_of(a) == 0xEF
    assert headings.allow_of(headings.parser().parse_args(["f"])) == 0xFF


@pytest.mark.parametrize("bad", [
    ["--top", "0"], ["--top", "17"], ["--min-blob-cells", "0"], ["--min-objects", ""], ["--min-objects", "0"], ["--min-objects", "2,2"],
    ["--allow", "X"], ["--ignore", "EAST"], ["--allow", "E", "--ignore", "W"], ["--top", "2", "--min-objects", "1,3"], ["--keep"],
])
def test_headings_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(headings, "MotionScanner", boom)
    monkeypatch.setattr(headings.tune, "load", boom)
    monkeypatch.setattr(headings.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        headings.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_headings_missing_geometry_exits_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(headings, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height / duration
    with pytest.raises(SystemExit) as ei:
        headings.main([path])
    assert ei.value.code == 2
    assert headings.main([str(tmp_path / "nothing_here.json")]) == 1
