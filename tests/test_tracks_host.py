"""CPU tier: object tracks (include/mtgpu_tracks.h) exist at every layer — header, library, ctypes table, Python module,
command, example — and reject bad arguments before any HIP call; the sequential model (tests/tracks_model.py) returns
every hand value of tests/tracks_inputs.py, equals the persistence model at k = 1 (consequence A) and has the
consequences B, D and E on random draws; the generated batches of the GPU tier are what they claim; the new kernel unit
compiles to three kernels without scratch and without a spilled VGPR.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, tracks

import persist_inputs as pi
import persist_model as pm
import tracks_inputs as ti
import tracks_model as tm
from test_derived_kernel_resources_host import compile_unit
from test_scan_kernel_resources_host import CSRC, makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mtgpu_track_objects", "mtgpu_track_objects_device", "mtgpu_tracks_preview"]
ALL = ("pred", "age", "id", "len", "track", "flags")


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_tracks.h")).read()


def model(c, **kw):
    a = ti.settings(c)
    a.update(kw)
    return tm.tracks(c["flags"], c["lists"], c["soff"], c["sd"], **a)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_TRACKS)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_TRACKS[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
    top = open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert top.count('#include "mtgpu_tracks.h"') == 1 and not any(n in top for n in NEW_SYMBOLS)
    assert _abi.ABI_TRACKS in _abi.ABI_TABLES
    assert C.sizeof(_abi.TracksPlanC) == 12
    assert [f for f, _ in _abi.TracksPlanC._fields_] == ["workgroup", "frames_per_tile", "work_words_per_entry"]
    assert (_abi.TRACK_NO_PRED, _abi.TRACK_NO_ID) == (0xFF, 0xFFFFFFFF) == (tm.NO_PRED, tm.NO_ID) == (tracks.NO_PRED, tracks.NO_ID)
    assert "#define MT_TRACK_NO_PRED 0xFFu" in hdr and "#define MT_TRACK_NO_ID 0xFFFFFFFFu" in hdr
    # the header states the consequences the tests rest on, the missing in-place form, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("A. k = 1, min_cells <= 1, and every M frame has list[f].cells > 0", "age[f] == pos[f], len[f] == track[f] == run[f]",
                 "persistence counts a run of 1 for that frame, this call gives track = 0", "B. For present entries: pred == 0xFF iff age == 1",
                 "The number of roots is the number of tracks", "C. For a level L >= 1", "One pass answers every MIN_TRACK",
                 "D. A stream's outputs from a call on that stream alone", "E. pred depends on reach, max_dropout, min_cells and the two lists only",
                 "Raising max_dropout turns no pred into none", "NO monotony in reach for age", "an unsorted list is legal input",
                 "It is not a matching", "NO in-place form", "Out of scope: exclusive (one-to-one) assignment", "velocity prediction",
                 "per-object direction", "the pipe, the C++ host layer and mtgpu_scan_file", "a compensated form",
                 "n_frames k must be below 0xFFFFFFFF", "takes nothing from the context's scratch ring"):
        assert text in flat, text
    src = open(os.path.join(CSRC, "tracks_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "#error" in src and "extern __shared__" not in src
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "tracks_kernels.hip" in mk and "tracks_kernels.h " in mk and "mtgpu_tracks.h" in mk
    blob = open(_abi.LIB_PATH, "rb").read()
    for name in (b"tracks_clear_kernel", b"tracks_streams_kernel", b"tracks_finish_kernel"):
        assert name in blob, name


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_tracks_plan p;\n"
            "  mt_object o = {0, 0, 0, 0, 0, 0};\n"
            "  return mtgpu_tracks_preview(MT_OBJECTS_MAX, &p)\n"
            "       + mtgpu_track_objects_device(c, 0, 0, &o, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0)\n"
            "       + mtgpu_track_objects(c, 0, 0, &o, 1, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0)\n"
            "       + p.workgroup + p.frames_per_tile + p.work_words_per_entry + (int)(MT_TRACK_NO_PRED + MT_TRACK_NO_ID);\n}\n")
    for first in ("mtgpu.h", "mtgpu_tracks.h", "mtgpu_objects.h", "mtgpu_persist.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_objects.h"\n#include "mtgpu_tracks.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/tracks_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "tracks_example.c")])


def test_canary_program_builds(tmp_path):
    """The plain-C contract program of the GPU tier compiles and links against the ABI (it cannot run without a device)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_tracks_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_tracks_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_module_is_the_python_layer():
    """The Python layer lives in mvtrim_amd.tracks: MotionScanner's methods and the package's export list are a recorded
    surface (tests/golden/scanner_calls.json) and stay what they were."""
    assert tracks.OUTPUTS == ALL and tracks.NO_PRED == 0xFF and tracks.NO_ID == 0xFFFFFFFF
    assert not hasattr(m.MotionScanner, "link") and not hasattr(m.MotionScanner, "track_objects") and "tracks" not in m.__all__
    for name in ("preview", "link", "link_device", "main", "measure", "parser", "histogram"):
        assert callable(getattr(tracks, name)), name
    from mvtrim_amd import scanner
    for name in ALL:
        assert name in scanner._OUTPUTS, name                 # the one output table holds the new rows


def test_preview_works_without_a_device():
    lib = m.load_library()
    for k in (1, 4, 16):
        p = _abi.TracksPlanC()
        assert lib.mtgpu_tracks_preview(k, C.byref(p)) == _abi.MT_OK
        assert p.workgroup > 0 and p.workgroup % 64 == 0 and p.frames_per_tile > 0 and (p.frames_per_tile * 16) % p.workgroup == 0
        assert p.work_words_per_entry == _abi.TRACK_WORK_WORDS == 2
        assert tracks.preview(k) == {"workgroup": p.workgroup, "frames_per_tile": p.frames_per_tile, "work_words_per_entry": 2}
    assert lib.mtgpu_tracks_preview(4, None) == _abi.MT_ERR_INVALID and "out" in lib.mtgpu_last_error().decode()
    for k in (0, 17, -1):
        assert lib.mtgpu_tracks_preview(k, C.byref(_abi.TracksPlanC())) == _abi.MT_ERR_INVALID and "k is %d" % k in lib.mtgpu_last_error().decode()
        with pytest.raises(m.MtgpuError):
            tracks.preview(k)


# ------------------------------------------------------------------ the kernel unit

def test_the_unit_holds_three_kernels_without_scratch(tmp_path):
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    res = compile_unit(("tracks", hipcc, flags, str(tmp_path / "tracks_kernels.o")))[1]
    for n, r in sorted(res.items()):
        print(n, r)
    assert len(res) == 3, sorted(res)
    for kernel in ("tracks_clear_kernel", "tracks_streams_kernel", "tracks_finish_kernel"):
        (r,) = [r for n, r in res.items() if kernel in n]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (kernel, r)
        assert r["LDS Size"] <= 8192, (kernel, r)                # static LDS of a few KB; no dynamic LDS is asked for at launch
    src = open(os.path.join(CSRC, "tracks_kernels.hip")).read()
    assert src.count("dim3(TB), 0, L.stream") == 3               # every launch: 0 bytes of dynamic LDS


# ------------------------------------------------------------------ arguments that need no device

def test_argument_errors_need_no_device():
    """What the arguments alone decide is answered before the context is looked at (ctx NULL here), with the argument
    named, and no byte of any buffer changes."""
    lib = m.load_library()
    buf = np.full(1024, 7, dtype=np.uint64)
    at = lambda byte: C.c_void_p(buf.ctypes.data + byte)      # noqa: E731
    # 8 frames, k = 2: nothing overlaps.  flags 8 B, has_sd 8 B, list 256 B, stream_off 16 B, work 128 B, pred 16 B,
    # age / id / len 64 B each, track 32 B, flags_out 8 B
    FL, SD, LI, SO, WK, PR, AG, ID, LN, TR, FO = (at(o) for o in (0, 64, 256, 512, 1024, 1280, 1536, 1792, 2048, 2304, 2560))
    OUTS = (PR, AG, ID, LN, TR, FO)

    def dev(flags=FL, sd=None, li=LI, k=2, n=8, soff=SO, ns=1, reach=1, work=WK, outs=OUTS):
        rc = lib.mtgpu_track_objects_device(None, flags, sd, li, k, n, soff, ns, 1, 0, reach, 1, work, *outs, None)
        return rc, lib.mtgpu_last_error().decode()

    def only(i, p):
        return tuple(p if j == i else None for j in range(6))

    for kw, word in ((dict(outs=(None,) * 6), "d_pred, d_age, d_id, d_len, d_track and d_flags_out are all NULL"),
                     (dict(k=0), "k is 0"), (dict(k=17), "k is 17"), (dict(k=-2), "k is -2"),
                     (dict(n=0xFFFFFFFF // 3, k=3), "not below 4294967295"), (dict(n=0xFFFFFFFF, k=1), "not below 4294967295"),
                     (dict(reach=65536), "reach"), (dict(flags=None), "d_flags is NULL"), (dict(li=None), "d_list is NULL"),
                     (dict(soff=None), "d_stream_off is NULL"), (dict(work=None), "d_work is NULL"), (dict(ns=0), "n_streams"),
                     (dict(soff=at(516)), "d_stream_off must be 8-byte aligned"), (dict(li=at(264)), "d_list must be 16-byte aligned"),
                     (dict(li=at(260)), "d_list must be 16-byte aligned"), (dict(work=at(1026)), "d_work must be 4-byte aligned"),
                     (dict(outs=only(1, at(1538))), "d_age must be 4-byte aligned"), (dict(outs=only(2, at(1793))), "d_id must be 4-byte aligned"),
                     (dict(outs=only(3, at(2050))), "d_len must be 4-byte aligned"), (dict(outs=only(4, at(2306))), "d_track must be 4-byte aligned"),
                     (dict(outs=only(5, FL)), "d_flags_out overlaps d_flags"), (dict(outs=only(5, at(7))), "d_flags_out overlaps d_flags"),
                     (dict(sd=SD, outs=only(0, at(71))), "d_pred overlaps d_has_sd"), (dict(outs=only(1, at(508))), "d_age overlaps d_list"),
                     (dict(outs=only(4, at(524))), "d_track overlaps d_stream_off"), (dict(work=at(4)), "d_work overlaps d_flags"),
                     (dict(outs=only(3, at(1024 + 64))), "d_len overlaps d_work"), (dict(outs=(None, AG, at(1596), None, None, None)), "d_id overlaps d_age"),
                     (dict(outs=(PR, None, None, None, None, at(1295))), "d_flags_out overlaps d_pred"), ({}, "ctx")):
        rc, msg = dev(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)
    # buffers that touch without sharing a byte are fine: only the context is missing
    rc, msg = dev(work=at(8), outs=(at(136), at(152), at(1536), at(1792), at(2048), at(216)), li=at(256), soff=at(224))
    assert rc == _abi.MT_ERR_INVALID and msg.startswith("ctx"), msg
    # n_frames == 0 asks for nothing but an output and a context
    assert dev(flags=None, li=None, soff=None, work=None, n=0, ns=0)[1].startswith("ctx")
    assert "all NULL" in dev(n=0, outs=(None,) * 6)[1]

    def host(flags=FL, li=at(257), k=2, n=8, soff=np.array([0, 8], dtype=np.uint64), ns=1, reach=1, outs=OUTS):
        rc = lib.mtgpu_track_objects(None, flags, None, li, k, n, None if soff is None else soff.ctypes.data_as(C.c_void_p), ns, 1, 0, reach, 1, *outs)
        return rc, lib.mtgpu_last_error().decode()
    for kw, word in ((dict(outs=(None,) * 6), "pred, age, id, len, track and flags_out are all NULL"), (dict(k=0), "k is 0"), (dict(k=17), "k is 17"),
                     (dict(flags=None), "flags is NULL"), (dict(li=None), "list is NULL"), (dict(soff=None), "stream_off is NULL"),
                     (dict(ns=0), "n_streams"), (dict(reach=70000), "reach"), (dict(outs=only(5, FL)), "flags_out overlaps flags"),
                     (dict(soff=np.array([0, 5, 3], dtype=np.uint64), ns=2), "stream_off not monotonic at stream 1"),
                     (dict(soff=np.array([0, 9], dtype=np.uint64)), "above n_frames"), ({}, "ctx")):      # `list` needs no alignment here
        rc, msg = host(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)
    assert (buf == 7).all()


# ------------------------------------------------------------------ the model against the hand values

@pytest.mark.parametrize("k", ti.HAND_K)
def test_model_returns_every_hand_value(k):
    for name in ti.HAND:
        c, hand = ti.hand_case(name, k)
        got = model(c)
        for o in ALL:
            assert got[o].tolist() == hand[o].tolist(), (name, o)
        e, sl, moved = ti.embed(c, hand, k)                  # as stream 2 of 4: the ids move (D)
        got = model(e)
        for o in ALL:
            assert got[o][sl].tolist() == moved[o].tolist(), (name, o)
    assert set(ti.HAND) >= {"chain", "split", "merge", "merge absent", "no box", "reach wide", "reach short", "reach 0", "dropout at limit",
                            "dropout past limit", "key frame", "empty list"}


def test_hand_values_say_what_their_names_say():
    c, w = ti.hand_case("split", 2)
    assert w["pred"][1].tolist() == [0, 0] and w["id"][1].tolist() == [0, 0]
    c, w = ti.hand_case("merge", 2)
    assert w["pred"][1, 0] == 0 and w["len"][0].tolist() == [2, 1]
    c, w = ti.hand_case("merge absent", 16)
    assert w["pred"][1, 0] == 1 and w["id"][1, 0] == 1 and c["lists"]["cells"][0, 0] < c["min_cells"] <= c["lists"]["cells"][0, 1]
    c, w = ti.hand_case("reach wide", 1)
    assert c["reach"] == 65535 and int(c["lists"]["x1"][0, 0]) + c["reach"] > 0xFFFF and w["age"][:, 0].tolist() == [1, 2, 3]
    c, w = ti.hand_case("empty list", 15)
    assert (c["flags"] != 0).all() and w["track"].tolist() == [1, 0, 1]


# ------------------------------------------------------------------ consequence A: the persistence model at k = 1

@pytest.mark.parametrize("name", list(pi.WORKED))
def test_k1_is_persistence_on_the_worked_cases(name):
    pc, run, pos, flags_out = pi.WORKED[name]
    c, _box = ti.persist_twin(pc)
    got = model(c)
    assert got["age"][:, 0].tolist() == pos and got["len"][:, 0].tolist() == run and got["track"].tolist() == run and got["flags"].tolist() == flags_out


@pytest.mark.parametrize("chunk", range(4))
def test_k1_is_persistence_on_random_draws(chunk):
    for seed in range(chunk * 25, chunk * 25 + 25):
        pc = pi.random_case(seed)
        c, box = ti.persist_twin(pc)
        got = model(c)
        want = pm.persist(pc["flags"], pc["soff"], pc["sd"], box, c["min_track"], c["max_dropout"], c["reach"])
        assert np.array_equal(got["age"][:, 0], want["pos"]) and np.array_equal(got["len"][:, 0], want["run"]), seed
        assert np.array_equal(got["track"], want["run"]) and np.array_equal(got["flags"], want["flags"]), seed
        if pc["box"] is None:                                # the constant box at any reach is persistence without boxes
            plain = pm.persist(pc["flags"], pc["soff"], pc["sd"], None, c["min_track"], c["max_dropout"])
            assert np.array_equal(want["run"], plain["run"]), seed
    # where an M frame's entry is absent the two differ, as the header says: persistence counts a run of 1, tracks give 0
    c = ti.case([1, 1, 1], ti.lists_of([[ti.A], [], [ti.A]], 1))
    assert model(c)["track"].tolist() == [1, 0, 1]
    assert pm.persist([1, 1, 1], [0, 3], None, pi.boxes([ti.A[2:], ti.EMPTY[2:], ti.A[2:]]))["run"].tolist() == [1, 1, 1]


# ------------------------------------------------------------------ consequences B, D, E on random draws

@pytest.mark.parametrize("chunk", range(4))
def test_model_has_the_consequences_on_random_draws(chunk):
    for seed in range(chunk * 15, chunk * 15 + 15):
        c = ti.random_case(seed)
        got = model(c)
        n, k = c["lists"].shape
        need = max(1, c["min_cells"])
        inside = np.zeros(n, dtype=bool)
        for s in range(len(c["soff"]) - 1):
            inside[int(c["soff"][s]):int(c["soff"][s + 1])] = True
        present = ((c["flags"] != 0) & inside)[:, None] & (c["lists"]["cells"] >= need)
        # the empty values
        assert (got["pred"][~present] == tm.NO_PRED).all() and (got["age"][~present] == 0).all() and (got["len"][~present] == 0).all(), seed
        assert (got["id"][~present] == tm.NO_ID).all() and (got["id"][present] != tm.NO_ID).all(), seed
        # B
        assert np.array_equal((got["pred"] == tm.NO_PRED) & present, (got["age"] == 1)), seed
        assert (got["len"] >= got["age"]).all(), seed
        roots = np.flatnonzero((got["age"] == 1).reshape(-1))
        assert np.array_equal(got["id"].reshape(-1)[roots], roots.astype(np.uint32)), seed                  # a root's id is its own index
        assert sorted(set(got["id"][present].tolist())) == roots.tolist(), seed                              # roots <-> tracks
        for r in roots:
            members = got["id"] == r
            assert (got["len"][members] == got["age"][members].max()).all(), seed                            # constant, and the largest age
        assert np.array_equal(got["track"], np.where(present, got["len"], 0).max(axis=1)), seed
        assert np.array_equal(got["flags"], ((c["flags"] != 0) & (got["track"] >= max(1, c["min_track"]))).astype(np.uint8)), seed
        # D
        for sl, one in ti.single_streams(c):
            alone = model(one)
            moved = np.where(alone["id"] == tm.NO_ID, tm.NO_ID, alone["id"].astype(np.int64) + sl.start * k).astype(np.uint32)
            assert np.array_equal(moved, got["id"][sl]), seed
            for o in ("pred", "age", "len", "track", "flags"):
                assert np.array_equal(alone[o], got[o][sl]), (seed, o)
        # E: a larger max_dropout turns no pred into none; pred does not depend on min_track
        for md in (min(c["max_dropout"] + 1, ti.NO_LIMIT), ti.NO_LIMIT):
            more = model(c, max_dropout=md)
            assert (more["pred"][got["pred"] != tm.NO_PRED] != tm.NO_PRED).all(), (seed, md)
        assert np.array_equal(model(c, min_track=9)["pred"], got["pred"]), seed


def test_no_monotony_in_reach_for_age():
    """The header claims none, and here is why: at reach 0 the object continues its own three-frame chain; at reach 4 it is
    also linked to a lower-ranked entry that appeared a frame ago, and follows that one."""
    far = ti.obj(9, 12, 2, 13, 3)                            # four cells from where `near` will be a frame later, six from where it was
    near = [ti.obj(4, 20 - f, 2, 21 - f, 3) for f in range(4)]
    frames = [[ti.EMPTY, near[0]], [ti.EMPTY, near[1]], [far, near[2]], [ti.EMPTY, near[3]]]
    c = ti.case([1, 1, 1, 1], ti.lists_of(frames, 2), reach=0)
    assert model(c)["age"][3].tolist() == [0, 4] and model(c, reach=4)["age"][3].tolist() == [0, 2]
    assert model(c)["pred"][3].tolist() == [tm.NO_PRED, 1] and model(c, reach=4)["pred"][3].tolist() == [tm.NO_PRED, 0]


def test_random_draws_cover_their_ranges():
    cs = [ti.random_case(s) for s in range(60)]
    assert {c["lists"].shape[1] for c in cs} == {1, 2, 3, 4, 7, 15, 16}
    assert any(c["sd"] is None for c in cs) and any(c["sd"] is not None for c in cs)
    got = [model(c) for c in cs]
    assert any((g["pred"] > 0)[g["pred"] != tm.NO_PRED].any() for g in got)           # links to other ranks than 0
    assert any(g["track"].max() >= 10 for g in got) and any((g["age"] == 1).sum() > 50 for g in got)
    unsorted = [c for c in cs if c["lists"].shape[1] > 1 and (np.diff(c["lists"]["cells"].astype(np.int64), axis=1) > 0).any()]
    assert len(unsorted) > 30                                                          # the lists are not ranked
    shared = 0
    for c, g in zip(cs, got):                                                          # splits: two entries of a frame with one predecessor
        p = np.sort(g["pred"].astype(np.int64), axis=1)
        shared += int(((p[:, 1:] == p[:, :-1]) & (p[:, 1:] != tm.NO_PRED)).any(axis=1).sum()) if p.shape[1] > 1 else 0
    assert shared > 20


# ------------------------------------------------------------------ the GPU tier's generated batches are what they claim

def test_seam_cases_sit_on_their_seams():
    T = tracks.preview(16)["frames_per_tile"]
    for k in (1, 2, 16):
        cases = ti.seam_cases(T, k)
        assert len(cases) == 14
        for n in (T - 1, T, T + 1, 2 * T + 1):
            c = cases[f"steady {n}"]
            got = model(c)
            assert len(c["flags"]) == n and got["track"].tolist() == [n] * n and got["age"][:, 0].tolist() == list(range(1, n + 1))
            if k > 1:
                assert (got["len"][::3, 1] == 1).all()                      # the far entry never links
            got = model(cases[f"gaps {n}"])
            assert got["track"].max() > T // 2 and (got["age"][:, 0] == 1).sum() == 1
        got = model(cases["tile of quiet"])
        assert got["track"][[3, 4, T + 40, T + 41]].tolist() == [4] * 4 and got["pred"][T + 40, 0] == 0
        got = model(cases["tile of quiet, bounded"])
        assert got["track"][[3, 4, T + 40, T + 41]].tolist() == [2] * 4 and got["pred"][T + 40, 0] == tm.NO_PRED
        for s in (16, 64, T, 2 * T):
            got = model(cases[f"split@{s}"])
            assert got["age"][s, 0] == s + 1 and got["pred"][s, 0] == 0
            if k > 1:
                assert got["pred"][s, 1] == 0 and got["age"][s, 1] == s + 1 and (s == 2 * T or got["pred"][s + 1, 1] == 1)


def test_streams_case_has_the_listed_streams():
    T = tracks.preview(16)["frames_per_tile"]
    c, lens = ti.streams_case(T, 3)
    assert len(lens) == 70 and lens[:8] == [0, 1, 2, 16, T + 1, 0, 0, 1] and int(c["soff"][0]) == 3
    assert len(c["flags"]) == int(c["soff"][-1]) + 5 and np.diff(c["soff"].astype(np.int64)).tolist() == lens
    got = model(c)
    outside = np.r_[0:3, int(c["soff"][-1]):len(c["flags"])]
    assert (c["flags"][outside] != 0).all() and (c["lists"]["cells"][outside] > 0).any()
    assert (got["id"][outside] == tm.NO_ID).all() and not got["track"][outside].any() and not got["flags"][outside].any()
    assert got["track"].max() > 3


def test_example_lists_give_the_examples_counts():
    frames = [([ti.obj(6, 2 + f, 2, 4 + f, 3)] if f <= 5 else []) + ([ti.obj(4, 20, 4 + f, 21, 5 + f)] if 2 <= f <= 9 else []) +
              ([ti.obj(2, 30, 15, 31, 15)] if f == 11 else []) for f in range(12)]
    fl = np.array([len(e) > 0 for e in frames], dtype=np.uint8)
    c = ti.case(fl, ti.lists_of(frames, 4))
    got = model(c)
    assert sorted(set(got["id"].ravel().tolist())) == [0, 9, 44, tm.NO_ID] and got["pred"][6, 0] == 1
    assert [int(model(c, min_track=lv)["flags"].sum()) for lv in (1, 2, 7, 9)] == [11, 10, 8, 0]
    src = open(os.path.join(ROOT, "examples", "tracks_example.c")).read()
    assert "kept[0] != 11 || kept[1] != 10 || kept[2] != 8 || kept[3] != 0" in src


# ------------------------------------------------------------------ the command's options

def test_tracks_options_parse():
    a = tracks.parser().parse_args(["f.mtmv", "--top", "4", "--min-blob-cells", "3", "--min-track", "2,7", "--max-dropout", "4294967295", "--reach", "3",
                                    "--keep", "cam.mtkeep", "--json", "--width", "1920", "--height", "1080", "--duration", "12.5"])
    assert (a.top, a.min_blob_cells, a.min_track, a.max_dropout, a.reach, a.keep, a.json) == (4, 3, [2, 7], 0xFFFFFFFF, 3, "cam.mtkeep", True)
    a = tracks.parser().parse_args(["f"])
    assert (a.top, a.min_blob_cells, a.min_track, a.max_dropout, a.reach, a.keep, a.json) == (16, 1, [1, 2, 3, 5], 0, 1, None, False)
    length = np.array([[3, 0], [3, 1], [3, 0], [12, 0]], dtype=np.uint32)
    pred = np.array([[255, 255], [0, 255], [0, 255], [255, 255]], dtype=np.uint8)
    age = np.array([[1, 0], [2, 1], [3, 0], [1, 0]], dtype=np.uint32)
    assert tracks.histogram(length, pred, age) == {"1": 1, "2": 0, "3-4": 1, "5-9": 0, "10-29": 1, "30-99": 0, "100+": 0}


@pytest.mark.parametrize("bad", [
    ["--top", "0"], ["--top", "17"], ["--top", "x"], ["--min-blob-cells", "0"], ["--min-track", ""], ["--min-track", "a"], ["--min-track", "0"],
    ["--min-track", "2,2"], ["--min-track", "4294967296"], ["--min-track", ",".join(str(i) for i in range(1, 17))], ["--max-dropout", "-1"],
    ["--max-dropout", "4294967296"], ["--reach", "65536"], ["--reach", "-1"], ["--width", "x"], ["--device", "gpu"], ["--keep"],
])
def test_tracks_bad_options_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(tracks, "MotionScanner", boom)
    monkeypatch.setattr(tracks.tune, "load", boom)
    monkeypatch.setattr(tracks.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        tracks.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_tracks_missing_geometry_exits_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(tracks, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height / duration
    with pytest.raises(SystemExit) as ei:
        tracks.main([path])
    assert ei.value.code == 2
    assert tracks.main([str(tmp_path / "nothing_here.json")]) == 1
    assert tracks.main([path, "--width", "160", "--height", "160", "--duration", "1", "--keep", str(tmp_path / "none.mtkeep")]) == 1
