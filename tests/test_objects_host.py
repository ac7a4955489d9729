"""CPU tier: object lists (include/mtgpu_objects.h) exist at every layer — header, library, ctypes table, Python
package, command, example — size their launch with host arithmetic alone and reject bad arguments before any HIP call;
the numpy restatement (tests/objects_model.py) returns every hand-derived list of tests/objects_inputs.py and, entry 0,
the blob model's largest blob on every plane of tests/blob_planes.py; the new kernel unit compiles to three kernels
without scratch, without a spilled VGPR, at eight waves per SIMD."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, objects

import blob_planes as bp
import blobs_inputs as bi
import blobs_model as bm
import objects_inputs as oi
import objects_model as om
from test_derived_kernel_resources_host import compile_unit
from test_scan_kernel_resources_host import CSRC, makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_objects_preview", "mtgpu_scan_frames_objects", "mtgpu_scan_objects_device"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_objects.h")).read()


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_OBJECTS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_OBJECTS[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        at = hdr.index("int " + n + "(")          # every declaration names the reference lines it stands for
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert _abi.ABI_OBJECTS in _abi.ABI_TABLES
    assert C.sizeof(_abi.ObjectsPlanC) == 16
    assert [f for f, _ in _abi.ObjectsPlanC._fields_] == ["lds_bytes", "workgroup", "keep_words_per_row", "keep_words_per_stream"]
    assert _abi.OBJECT_DTYPE.itemsize == 16 and _abi.OBJECT_DTYPE.names == ("cells", "first", "x0", "y0", "x1", "y1")
    assert [_abi.OBJECT_DTYPE.fields[n][1] for n in _abi.OBJECT_DTYPE.names] == [0, 4, 8, 10, 12, 14]
    assert (_abi.OBJECTS_MAX, _abi.OBJECT_TABLE_BYTES) == (16, 24) == (om.K_MAX, oi.TABLE_BYTES)
    assert "#define MT_OBJECTS_MAX 16" in hdr and "#define MT_OBJECT_TABLE_BYTES 24" in hdr
    assert '#include "mtgpu_objects.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # the header states the consequences the GPU tests rest on, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("list[f k + 0] is the blob scan's largest[f] and box[f], bit for bit", "With min_objects <= 1, flags equals the blob scan's flags",
                 "The list for k is the first k entries of the list for MT_OBJECTS_MAX", "it equals centres when blobs <= k",
                 "objects <= blobs", "One scan answers every MIN_OBJECTS", "Raising min_blob_cells raises no objects[f]",
                 "counted over ALL blobs", "no pipe form", "no C++ host layer method", "no mtgpu_scan_file option", "no compensated form",
                 "no tracks across frames", "no per-object direction"):
        assert text in flat, text
    csrc = os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc")
    src = open(os.path.join(csrc, "objects_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "blobs_frames_kernel<" not in src
    for name in ("objects_kernels.hip", "objects_kernels.h", "blob_rank.h"):
        assert name in open(os.path.join(csrc, "Makefile")).read(), name
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"objects_frames_kernel" in blob and b"objects_clear_kernel" in blob


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_objects_plan p;\n"
            "  mt_object o = {0, 0, 0, 0, 0, 0};\n"
            "  return mtgpu_objects_preview(0, MT_OBJECTS_MAX, 163840, &p)\n"
            "       + mtgpu_scan_objects_device(c, 0, 40, 0, 0, 0, 0, 0, 0, 0, 4, 1, 1, 0, 0, 0, 0, &o, 0)\n"
            "       + mtgpu_scan_frames_objects(c, 0, 0, 0, 0, 0, 0, 0, 4, 1, 1, 0, 0, 0, 0, &o)\n"
            "       + p.lds_bytes + p.workgroup + p.keep_words_per_row + p.keep_words_per_stream + (int)(o.cells + o.first) + o.x0 + o.y0\n"
            "       + o.x1 + o.y1 + (int)sizeof(mt_object) + MT_OBJECT_TABLE_BYTES;\n}\n"
            "typedef char object_is_16_bytes[sizeof(mt_object) == 16 ? 1 : -1];\n")
    for first in ("mtgpu.h", "mtgpu_objects.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_objects.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/objects_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "objects_example.c")])


def test_canary_program_builds(tmp_path):
    """The plain-C contract program of the GPU tier compiles and links against the ABI (it cannot run without a device)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_objects_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_objects_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_package_exports_the_methods():
    """The Python layer lives in mvtrim_amd.objects: MotionScanner's methods and the package's export list are a recorded
    surface (tests/golden/scanner_calls.json) and stay what they were."""
    assert objects.OBJECT_DTYPE is _abi.OBJECT_DTYPE and objects.OUTPUTS == ("flags", "centres", "blobs", "objects", "list")
    assert not hasattr(m.MotionScanner, "scan_objects") and "objects" not in m.__all__
    for name in ("preview", "scan", "scan_device", "main", "measure", "parser", "size_histogram"):
        assert callable(getattr(objects, name)), name


# ------------------------------------------------------------------ the kernel unit

@pytest.fixture(scope="module")
def unit_resources(tmp_path_factory):
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    assert os.path.exists(os.path.join(CSRC, "objects_kernels.hip"))
    return compile_unit(("objects", hipcc, flags, str(tmp_path_factory.mktemp("objects_res") / "objects_kernels.o")))[1]


def test_the_unit_holds_three_kernels_without_scratch_at_eight_waves(unit_resources):
    """Three kernels: the 40-byte and the 8-byte form of objects_frames_kernel and objects_clear_kernel — the design needs
    no pipe form and no third record form, and documents the clear as the third kernel of the unit.  No scratch, no
    spilled VGPR, eight waves per SIMD: the siblings' floor, which two 1080p workgroups per CU need."""
    for n, r in sorted(unit_resources.items()):
        print(n, r)
    frames = sorted(n for n in unit_resources if "objects_frames_kernel" in n)
    clear = [n for n in unit_resources if "objects_clear_kernel" in n]
    assert len(frames) == 2 and len(clear) == 1 and len(unit_resources) == 3, sorted(unit_resources)
    assert [bool(re.search(r"objects_frames_kernelILi1024ELi\d+ELi%dEE" % rec, n)) for n, rec in zip(frames, (40, 8))] == [True, True], frames
    assert not any("blobs_frames_kernel" in n for n in unit_resources)
    for n in frames + clear:
        r = unit_resources[n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["Occupancy"] >= 8, (n, r)


# ------------------------------------------------------------------ preview

def preview(params, k, lds=MI355X_LDS):
    p = _abi.ObjectsPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_objects_preview(C.byref(c), k, lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def test_preview_is_the_blob_layout_plus_the_table():
    for w, h, kw in [(1920, 1080, {}), (3840, 2160, {}), (3840, 2160, dict(vertical_mask=0.0)), (1280, 720, {}),
                     (48, 48, dict(vertical_mask=0.0)), (1920, 1080, dict(vertical_mask=0.5))]:
        params = m.ScanParams.from_config(w, h, **kw)
        blob = m.blobs_preview(params)
        R = max(1, params.grid_h - 2 * params.vertical_margin)
        for k in (1, 16):
            rc, p, msg = preview(params, k)
            assert rc == _abi.MT_OK, msg
            assert p.lds_bytes == blob["lds_bytes"] + k * 24 == oi.lds_by_hand(params.grid_w, R, k) <= MI355X_LDS
            assert (p.workgroup, p.keep_words_per_row, p.keep_words_per_stream) == (1024, blob["keep_words_per_row"], blob["keep_words_per_stream"])
            assert objects.preview(params, k) == {"lds_bytes": p.lds_bytes, "workgroup": 1024, "keep_words_per_row": p.keep_words_per_row,
                                                    "keep_words_per_stream": p.keep_words_per_stream}
    # two 1080p workgroups share a CU's LDS at k = 16
    assert 2 * objects.preview(m.ScanParams.from_config(1920, 1080), 16)["lds_bytes"] <= MI355X_LDS


def test_preview_refusals():
    lib = m.load_library()
    good = m.ScanParams.from_config(1920, 1080)
    c = good.to_c()
    inv = _abi.MT_ERR_INVALID
    for k in (0, -1, 17, 1 << 20):
        rc, _, msg = preview(good, k)
        assert rc == inv and "k is %d" % k in msg, (k, msg)
    assert lib.mtgpu_objects_preview(None, 4, MI355X_LDS, C.byref(_abi.ObjectsPlanC())) == inv
    assert lib.mtgpu_objects_preview(C.byref(c), 4, MI355X_LDS, None) == inv
    assert lib.mtgpu_objects_preview(C.byref(c), 4, 100, C.byref(_abi.ObjectsPlanC())) == inv
    # the grids the plain scan cuts into row bands have no form; nor has 1080p on a device with 16 KB
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2), 1)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0), 16)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    rc, _, msg = preview(good, 16, 16384)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "120x68" in msg and "16 objects" in msg
    with pytest.raises(m.MtgpuError) as ei:
        objects.preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2), 16)
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
    with pytest.raises(m.MtgpuError) as ei:
        objects.preview(good, 17)
    assert ei.value.code == inv


@pytest.mark.parametrize("k", range(1, 17))
def test_the_last_grid_each_k_accepts(k):
    """By bisection over the preview (the input of the GPU tier's cliff case): the tallest 65-column grid for k entries
    fits by the hand formula, one more row does not and is refused with the grid named; a larger k never accepts more."""
    gh = oi.cliff_rows(k)
    assert oi.lds_by_hand(65, gh, k) <= MI355X_LDS < oi.lds_by_hand(65, gh + 1, k)
    rc, p, msg = preview(bi.limit_params(65, gh), k)
    assert rc == _abi.MT_OK and p.lds_bytes == oi.lds_by_hand(65, gh, k), msg
    rc, _, msg = preview(bi.limit_params(65, gh + 1), k)
    assert rc == _abi.MT_ERR_UNSUPPORTED and f"65x{gh + 1}" in msg, msg
    assert gh <= bi.limit_shapes()["tall"][1] and (k == 1 or gh <= oi.cliff_rows(k - 1)) and gh > 500


# ------------------------------------------------------------------ error paths that need no device

def test_invalid_arguments_are_rejected_without_a_device():
    """Everything the arguments alone decide is answered before the context is looked at: no HIP call, no byte written."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(64)          # never dereferenced
    odd = C.c_void_p(68)

    def err():
        return lib.mtgpu_last_error().decode()

    def dev(rec=one, rb=40, nrec=1, off=one, n=1, soff=one, ns=1, keep=one, k=4, fl=one, ce=one, bl=one, ob=one, li=one):
        return lib.mtgpu_scan_objects_device(None, rec, rb, nrec, off, None, n, soff, ns, keep, k, 1, 1, fl, ce, bl, ob, li, None)

    for k in (0, 17, -3):
        assert dev(k=k) == inv and "k is %d" % k in err()
    for rb in (0, 7, 16, 39, 41, -8):
        assert dev(rb=rb) == inv and "rec_bytes" in err()
    assert dev(fl=None, ce=None, bl=None, ob=None, li=None) == inv and "all NULL" in err()
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
    assert dev(ob=C.c_void_p(66)) == inv and "d_objects" in err()
    for a in (65, 66, 68, 72):
        assert dev(li=C.c_void_p(a)) == inv and "d_list must be 16-byte aligned" in err(), a
    assert dev() == inv and "ctx" in err()
    assert dev(keep=None, soff=None, ns=0) == inv and "ctx" in err()         # the form without a mask is a valid one
    assert dev(k=16) == inv and "ctx" in err() and dev(k=1) == inv and "ctx" in err()

    out = np.full(3, 7, dtype=np.uint32)
    fl = np.full(3, 7, dtype=np.uint8)
    lst = np.full((3, 4, 16), 7, dtype=np.uint8)
    mv = np.zeros(8, dtype=m.MV_DTYPE)
    keep = np.zeros(4, dtype=np.uint64)
    good_off, good_soff = np.array([0, 4, 8], dtype=np.uint64), np.array([0, 2], dtype=np.uint64)

    def host(off=good_off, soff=good_soff, ns=1, kp=keep, k=4, f=fl, c=out, li=lst, recs=mv):
        return lib.mtgpu_scan_frames_objects(None, vp(recs), vp(off), None, 2, vp(soff), ns, vp(kp), k, 1, 1, vp(f), vp(c), None, None, vp(li))

    assert host(k=0) == inv and "k is 0" in err()
    assert host(k=17) == inv and "k is 17" in err()
    assert host(f=None, c=None, li=None) == inv and "all NULL" in err()
    assert host(soff=None) == inv and "stream_off" in err()
    assert host(off=None) == inv and "frame_off" in err()
    assert host(ns=0) == inv and "n_streams" in err()
    assert host(kp=None) == inv and "keep is NULL" in err()
    assert host(kp=None, soff=None) == inv and "n_streams" in err()
    assert host(off=np.array([0, 9, 8], dtype=np.uint64)) == inv and "frame_off not monotonic" in err()
    assert host(soff=np.array([0, 2, 1], dtype=np.uint64), ns=2) == inv and "stream_off not monotonic" in err()
    assert host(soff=np.array([0, 1], dtype=np.uint64)) == inv and "stream_off[1]" in err() and "n_frames" in err()
    assert host(recs=None) == inv and "mv is NULL" in err()
    assert host() == inv and "ctx" in err()
    assert host(kp=None, soff=None, ns=0) == inv and "ctx" in err()
    assert out.tolist() == [7, 7, 7] and fl.tolist() == [7, 7, 7] and (lst == 7).all()


# ------------------------------------------------------------------ the model

def test_model_on_hand_planes():
    """Values written out here: a tie decided by `first`, a blob that is larger although it starts later, the box of an
    L, single cells (no centres), empties behind the last blob."""
    p = bi.grid(20, 12)
    #   A  (10, 2) (11, 2) (10, 3)     3 cells, first 2 * 20 + 10 = 50
    #   B  (3, 6) (4, 6) (5, 6)        3 cells, first 6 * 20 + 3 = 123: the tie goes to A, although B lies further left
    #   C  (14, 8) .. (17, 8), (17, 9) 5 cells, first 8 * 20 + 14 = 174: the largest, although it starts last
    #   (1, 1) alone: active, no centre
    A, B = [(10, 2), (11, 2), (10, 3)], [(3, 6), (4, 6), (5, 6)]
    Cc = [(14, 8), (15, 8), (16, 8), (17, 8), (17, 9)]
    mv, off, sd = bi.batch_of([bi.cells_frame(A + B + Cc + [(1, 1)]), None, bi.cells_frame(A + B)], 7)
    want0 = [(5, 174, 14, 8, 17, 9), (3, 50, 10, 2, 11, 3), (3, 123, 3, 6, 5, 6)]
    assert om.ranked(bm.centre_plane(p, mv[int(off[0]):int(off[1])])) == want0
    for k in (1, 2, 3, 4, 16):
        r = om.model_batch(p, mv, off, sd, k, 3)
        assert r["centres"].tolist() == [11, 0, 6] and r["blobs"].tolist() == [3, 0, 2] and r["objects"].tolist() == [3, 0, 2]
        assert r["list"].shape == (3, k)
        assert r["list"][0].tolist() == (want0 + [om.EMPTY] * k)[:k]
        assert r["list"][1].tolist() == [om.EMPTY] * k
        assert r["list"][2].tolist() == (want0[1:] + [om.EMPTY] * k)[:k]
    assert om.model_batch(p, mv, off, sd, 2, 4)["objects"].tolist() == [1, 0, 0]           # counted over all blobs, k = 2 or not
    assert om.model_batch(p, mv, off, sd, 1, 1)["objects"].tolist() == [3, 0, 2]
    assert om.flags_np(p, [11, 0, 6], [3, 0, 2], 3).tolist() == [1, 0, 0]


def test_every_hand_list_holds_on_the_model():
    c = oi.hand_case()
    for masked in (False, True):
        hand = c.hand["masked" if masked else "plain"]
        for k in (1, 2, 3, 16):
            for mbc in (1, 3, 4):
                got = om.model_batch(c.p, c.mv, c.off, c.sd, k, mbc, c.soff if masked else None, c.keeps if masked else None)
                want = oi.hand_want(hand, k, mbc)
                for n in want:
                    assert got[n].tolist() == want[n].tolist(), (masked, k, mbc, n)
    assert oi.hand_want(c.hand["plain"], 16, 3)["objects"].tolist() == [2, 0, 0, 2]
    for case in (oi.pairs_case(), oi.seams_case()):
        got = om.model_batch(case.p, case.mv, case.off, case.sd, 16, 2)
        want = oi.hand_want(case.hand, 16, 2)
        for n in want:
            assert got[n].tolist() == want[n].tolist(), n
    p = oi.pairs_case()
    assert len(p.hand[0][2]) == 21 and om.model_batch(p.p, p.mv, p.off, p.sd, 16, 2)["objects"].tolist() == [21]
    assert om.model_batch(p.p, p.mv, p.off, p.sd, 16, 3)["objects"].tolist() == [0]
    assert [e[0] for e in oi.seams_case().hand[0][2]] == [38, 31, 16, 11]


def test_stream_input_counts_what_it_says():
    p, mv, off, sd, pts, soff = oi.streams_case()
    want = om.model_batch(p, mv, off, sd, 16, oi.SWEEP_MIN_BLOB)
    assert want["objects"].tolist() == oi.stream_objects().tolist() == want["blobs"].tolist()
    assert sorted(set(want["objects"].tolist())) == [0, 1, 2, 3, 4, 5]
    # F: raising min_blob_cells raises no objects[f]; the list stays
    prev = want
    for mbc in (3, 4, 5):
        nxt = om.model_batch(p, mv, off, sd, 16, mbc)
        assert (nxt["objects"] <= prev["objects"]).all() and nxt["list"].tolist() == want["list"].tolist()
        assert nxt["objects"].tolist() == om.objects_at(want, mbc).tolist()
        prev = nxt
    assert int(prev["objects"].max()) == 0


@pytest.mark.parametrize("name", bp.BATCHES)
def test_entry_0_is_the_blob_models_largest_blob(name):
    """On every plane of blob_planes: entry 0 == blobs_model.blob_stats' largest and box (bp.expected), centres and blobs
    equal, and the identities of consequence D."""
    want, blob = oi.expected(name), bp.expected(name)
    lst = want["list"]
    assert want["centres"].tolist() == blob["centres"].tolist() and want["blobs"].tolist() == blob["blobs"].tolist()
    assert lst["cells"][:, 0].tolist() == blob["largest"].tolist()
    box = np.stack([lst[n][:, 0] for n in ("x0", "y0", "x1", "y1")], axis=1)
    assert box.tolist() == blob["box"].tolist()
    cells = lst["cells"].astype(np.int64)
    total = cells.sum(axis=1)
    few = want["blobs"] <= om.K_MAX
    assert (total <= want["centres"]).all() and (total[few] == want["centres"][few]).all()
    assert (want["objects"] == want["blobs"]).all()                        # min_blob_cells 1
    assert ((cells > 0).sum(axis=1) == np.minimum(want["blobs"], om.K_MAX)).all()
    key = cells * (1 << 32) + (0xFFFFFFFF - lst["first"].astype(np.int64))
    assert (np.diff(key, axis=1)[cells[:, 1:] > 0] < 0).all()                # strictly ordered where listed
    if "confetti" in bp.batch(name).names:
        f = bp.batch(name).frame_of["confetti"]
        assert set(cells[f].tolist()) == {3} and (np.diff(lst["first"][f].astype(np.int64)) > 0).all()


# ------------------------------------------------------------------ the command

def test_objects_options_parse():
    a = objects.parser().parse_args(["f.mtmv", "--top", "4", "--min-blob-cells", "3", "--min-objects", "1,2,5", "--keep", "cam.mtkeep", "--json",
                                     "--width", "1920", "--height", "1080", "--duration", "12.5", "--vertical-mask", "0"])
    assert (a.top, a.min_blob_cells, a.min_objects, a.keep, a.json) == (4, 3, [1, 2, 5], "cam.mtkeep", True)
    a = objects.parser().parse_args(["f"])
    assert (a.top, a.min_blob_cells, a.min_objects, a.keep, a.json) == (16, 1, [1, 2, 3], None, False)
    assert objects.size_histogram(np.array([[0, 1, 2], [3, 4, 7], [8, 63, 64], [200, 0, 0]], dtype=np.uint32)) == {
        "1": 1, "2-3": 2, "4-7": 2, "8-15": 1, "16-31": 0, "32-63": 1, "64+": 2}


@pytest.mark.parametrize("bad", [
    ["--top", "0"], ["--top", "17"], ["--top", "x"], ["--min-blob-cells", "0"], ["--min-blob-cells", "1,2"], ["--min-objects", ""],
    ["--min-objects", "a"], ["--min-objects", "0"], ["--min-objects", "2,2"], ["--min-objects", "4294967296"],
    ["--min-objects", ",".join(str(i) for i in range(1, 18))], ["--width", "x"], ["--device", "gpu"], ["--keep"],
])
def test_objects_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(objects, "MotionScanner", boom)
    monkeypatch.setattr(objects.tune, "load", boom)
    monkeypatch.setattr(objects.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        objects.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_objects_missing_geometry_exits_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(objects, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height / duration
    with pytest.raises(SystemExit) as ei:
        objects.main([path])
    assert ei.value.code == 2
    assert objects.main([str(tmp_path / "nothing_here.json")]) == 1
    assert objects.main([path, "--width", "160", "--height", "160", "--duration", "1", "--keep", str(tmp_path / "none.mtkeep")]) == 1
