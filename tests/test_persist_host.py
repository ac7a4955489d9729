"""CPU tier: temporal persistence (include/mtgpu_persist.h) exists at every layer — header, library, ctypes table, Python
methods, the `persist` command — and the checker of tests/test_gpu_persist.py is what it claims to be: the sequential
model returns every worked case of the header and has the consequences A-D, F and G on random streams, and the generated
batches have the properties their names promise.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, persist

import persist_inputs as pi
import persist_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mtgpu_persist_flags", "mtgpu_persist_flags_device", "mtgpu_persist_preview"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_persist.h")).read()


def model(c, **kw):
    a = dict(min_run=c["min_run"], max_dropout=c["max_dropout"], reach=c["reach"])
    a.update(kw)
    return pm.persist(c["flags"], c["soff"], c["sd"], c["box"], **a)


# ------------------------------------------------------------------ symbols, headers, example

def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_PERSIST)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_PERSIST[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
    top = open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    assert top.rstrip().endswith('#include "mtgpu_persist.h"\n\n#endif /* MTGPU_H */')        # included last
    assert not any(n in top for n in NEW_SYMBOLS)
    assert C.sizeof(_abi.PersistPlanC) == 8 and [f for f, _ in _abi.PersistPlanC._fields_] == ["workgroup", "frames_per_tile"]
    # the header states the consequences the tests rest on, the missing in-place form, and what is out of scope
    flat = " ".join(hdr.replace("*", " ").split())
    for text in ("A. min_run <= 1", "B. box == NULL and max_dropout = 0xFFFFFFFF", "C. box == NULL, has_sd == NULL, max_dropout = 0",
                 "D. Inside a run, pos counts 1 .. run", "E. For a level L >= 1", "F. Raising max_dropout or reach never lowers",
                 "G. A stream's outputs equal those of a call on that stream alone", "NO in-place form", "Out of scope: the pipe",
                 "run duration in seconds", "filling the bridged Q frames", "tracking more than the largest blob",
                 "takes nothing from the context's scratch ring"):
        assert text in flat, text
    src = open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "persist_kernels.hip")).read()
    assert "getenv" not in src and "__gfx950__" in src and "#error" in src and "atomic" not in src.replace("No global atomics", "")
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"persist_streams_kernel" in blob and b"persist_clear_kernel" in blob
    mk = open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "Makefile")).read()
    assert "persist_kernels.hip" in mk and "persist_kernels.h " in mk and "mtgpu_persist.h" in mk


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_persist_plan p;\n"
            "  mt_blob_box b = {0, 0, 0, 0};\n"
            "  return mtgpu_persist_preview(&p)\n"
            "       + mtgpu_persist_flags_device(c, 0, 0, &b, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0)\n"
            "       + mtgpu_persist_flags(c, 0, 0, &b, 0, 0, 0, 1, 0, 1, 0, 0, 0)\n"
            "       + p.workgroup + p.frames_per_tile;\n}\n")
    for first in ("mtgpu.h", "mtgpu_persist.h", "mtgpu_blobs.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_plain_c_example_compiles():
    """examples/persist_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "persist_example.c")])


def test_canary_program_builds(tmp_path):
    """The plain-C contract program of the GPU tier compiles and links against the ABI (it cannot run without a device)."""
    pkg = os.path.dirname(m.LIB_PATH)
    exe = str(tmp_path / "abi_persist_canaries")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "abi_persist_canaries.c"),
                           "-o", exe, "-L" + pkg, "-lmtgpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + pkg,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_package_exports_the_methods():
    for name in ("persist", "persist_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.persist_preview) and "persist_preview" in m.__all__


def test_preview_works_without_a_device():
    lib = m.load_library()
    p = _abi.PersistPlanC()
    assert lib.mtgpu_persist_preview(C.byref(p)) == _abi.MT_OK
    assert p.workgroup > 0 and p.workgroup % 64 == 0 and p.frames_per_tile > 0 and p.frames_per_tile % p.workgroup == 0
    assert m.persist_preview() == {"workgroup": p.workgroup, "frames_per_tile": p.frames_per_tile}
    assert lib.mtgpu_persist_preview(None) == _abi.MT_ERR_INVALID and "out" in lib.mtgpu_last_error().decode()


# ------------------------------------------------------------------ arguments that need no device

def test_argument_errors_need_no_device():
    """What the arguments alone decide is answered before the context is looked at (ctx NULL here), with the argument
    named."""
    lib = m.load_library()
    buf = np.zeros(256, dtype=np.uint64)
    at = lambda byte: C.c_void_p(buf.ctypes.data + byte)      # noqa: E731
    FL, SD, BX, SO, WK, FO, RU, PO = (at(o) for o in (0, 64, 128, 256, 512, 768, 1024, 1280))   # 8 frames: nothing overlaps

    def dev(flags=FL, sd=None, box=None, n=8, soff=SO, ns=1, reach=1, work=WK, outs=(FO, RU, PO)):
        rc = lib.mtgpu_persist_flags_device(None, flags, sd, box, n, soff, ns, 1, 0, reach, work, *outs, None)
        return rc, lib.mtgpu_last_error().decode()
    for kw, word in ((dict(outs=(None, None, None)), "all NULL"), (dict(flags=None), "d_flags"), (dict(soff=None), "d_stream_off"),
                     (dict(work=None), "d_work"), (dict(ns=0), "n_streams"), (dict(reach=65536), "reach"),
                     (dict(soff=at(260)), "d_stream_off must be 8-byte aligned"), (dict(box=at(129)), "d_box must be 2-byte aligned"),
                     (dict(work=at(514)), "d_work must be 4-byte aligned"), (dict(outs=(FO, at(1026), None)), "d_run must be 4-byte aligned"),
                     (dict(outs=(None, None, at(1281))), "d_pos must be 4-byte aligned"),
                     (dict(outs=(FL, None, None)), "d_flags_out overlaps d_flags"), (dict(outs=(at(7), None, None)), "d_flags_out overlaps d_flags"),
                     (dict(sd=SD, outs=(at(71), None, None)), "d_flags_out overlaps d_has_sd"),
                     (dict(box=BX, outs=(None, at(188), None)), "d_run overlaps d_box"),
                     (dict(outs=(None, at(268), None)), "d_run overlaps d_stream_off"), (dict(work=at(4)), "d_work overlaps d_flags"),
                     (dict(outs=(None, WK, None)), "d_run overlaps d_work"), (dict(outs=(None, RU, at(1052))), "d_pos overlaps d_run"),
                     (dict(outs=(at(1031), RU, None)), "d_run overlaps d_flags_out"), (dict(outs=(None, None, at(540))), "d_pos overlaps d_work"),
                     ({}, "ctx")):
        rc, msg = dev(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)
    # buffers that touch without sharing a byte are fine: only the context is missing
    rc, msg = dev(work=at(8), outs=(at(40), at(48), at(80)), soff=at(112))
    assert rc == _abi.MT_ERR_INVALID and "ctx" in msg, msg
    # n_frames == 0 asks for nothing but an output and a context
    assert dev(flags=None, soff=None, work=None, n=0, ns=0)[1].startswith("ctx")
    assert "all NULL" in dev(n=0, outs=(None, None, None))[1]

    def host(flags=FL, n=8, soff=np.array([0, 8], dtype=np.uint64), ns=1, reach=1, outs=(FO, RU, PO)):
        rc = lib.mtgpu_persist_flags(None, flags, None, None, n, None if soff is None else soff.ctypes.data_as(C.c_void_p), ns, 1, 0, reach, *outs)
        return rc, lib.mtgpu_last_error().decode()
    for kw, word in ((dict(outs=(None, None, None)), "all NULL"), (dict(flags=None), "flags is NULL"), (dict(soff=None), "stream_off is NULL"),
                     (dict(ns=0), "n_streams"), (dict(reach=70000), "reach"), (dict(outs=(FL, None, None)), "flags_out overlaps flags"),
                     (dict(soff=np.array([0, 5, 3], dtype=np.uint64), ns=2), "stream_off not monotonic at stream 1"),
                     (dict(soff=np.array([0, 9], dtype=np.uint64)), "above n_frames"), ({}, "ctx")):
        rc, msg = host(**kw)
        assert rc == _abi.MT_ERR_INVALID and word in msg, (kw, msg)


# ------------------------------------------------------------------ the model against the hand values

@pytest.mark.parametrize("name", list(pi.WORKED))
def test_model_returns_the_worked_cases(name):
    c, run, pos, flags_out = pi.WORKED[name]
    got = model(c)
    assert got["run"].tolist() == run and got["pos"].tolist() == pos and got["flags"].tolist() == flags_out
    # embedded as stream 3 of 5, the stream reads the same (G)
    e, sl = pi.embed(c)
    assert len(e["soff"]) == 6 and np.array_equal(e["flags"][sl], c["flags"])
    got = model(e)
    assert got["run"][sl].tolist() == run and got["pos"][sl].tolist() == pos and got["flags"][sl].tolist() == flags_out


def test_linked_is_the_headers():
    a = (10, 10, 12, 12)
    assert pm.linked(a, (14, 10, 16, 12), 2) and not pm.linked(a, (15, 10, 16, 12), 2) and pm.linked(a, (15, 10, 16, 12), 3)
    assert pm.linked((14, 10, 16, 12), a, 2) and not pm.linked((15, 10, 16, 12), a, 2)          # symmetric
    assert pm.linked(a, (10, 15, 12, 16), 3) and not pm.linked(a, (10, 16, 12, 16), 3)          # the rows alike
    assert not pm.linked(pm.NO_BOX, pm.NO_BOX, 65535) and not pm.linked(a, pm.NO_BOX, 65535) and not pm.linked(pm.NO_BOX, a, 65535)
    assert pm.linked((0, 0, 0, 0), (65535, 65535, 65535, 65534), 65535)                          # 32-bit arithmetic: no wrap at 16
    assert not pm.linked((0, 0, 0, 0), (65535, 65535, 65535, 65534), 65534)


# ------------------------------------------------------------------ consequences A-D, F, G on random draws

def m_counts(c):
    return [int((c["flags"][int(c["soff"][s]):int(c["soff"][s + 1])] != 0).sum()) for s in range(len(c["soff"]) - 1)]


def block_lengths(flags):
    """Per frame, the length of the maximal block of consecutive non-zero flags it lies in (0 on a zero flag)."""
    out = np.zeros(len(flags), dtype=np.uint32)
    f = 0
    while f < len(flags):
        g = f
        while g < len(flags) and flags[g] != 0:
            g += 1
        out[f:g] = g - f
        f = max(g, f + 1)
    return out


@pytest.mark.parametrize("chunk", range(8))
def test_model_has_the_consequences_on_random_draws(chunk):
    for seed in range(chunk * 25, chunk * 25 + 25):          # 200 draws
        c = pi.random_case(seed)
        got = model(c)
        is_m = c["flags"] != 0
        # A
        for mr in (0, 1):
            assert np.array_equal(model(c, min_run=mr)["flags"], is_m.astype(np.uint8)), seed
        assert np.array_equal(got["flags"], (is_m & (got["run"] >= max(1, c["min_run"]))).astype(np.uint8)), seed
        # B
        every = pm.persist(c["flags"], c["soff"], c["sd"], None, max_dropout=pi.NO_LIMIT)
        for s, cnt in enumerate(m_counts(c)):
            sl = slice(int(c["soff"][s]), int(c["soff"][s + 1]))
            assert np.array_equal(every["run"][sl], np.where(is_m[sl], cnt, 0)), seed
        # C
        plain = pm.persist(c["flags"], c["soff"], None, None, max_dropout=0)
        for s in range(len(c["soff"]) - 1):
            sl = slice(int(c["soff"][s]), int(c["soff"][s + 1]))
            assert np.array_equal(plain["run"][sl], block_lengths(c["flags"][sl])), seed
        # D
        assert np.array_equal(got["pos"] != 0, is_m) and np.array_equal(got["run"] != 0, is_m), seed
        assert (got["pos"] <= got["run"]).all() and int(got["run"][got["pos"] == 1].sum()) == int(is_m.sum()), seed
        idx = np.flatnonzero(is_m)
        for a, b in zip(idx[:-1], idx[1:]):                  # consecutive M frames: the run goes on or a new one starts
            same_stream = np.searchsorted(c["soff"], a, "right") == np.searchsorted(c["soff"], b, "right")
            if same_stream and got["pos"][b] != 1:
                assert got["pos"][b] == got["pos"][a] + 1 and got["run"][b] == got["run"][a], seed
            else:
                assert got["pos"][b] == 1 and got["pos"][a] == got["run"][a], seed
        if len(idx):
            assert got["pos"][idx[0]] == 1 and got["pos"][idx[-1]] == got["run"][idx[-1]], seed
        # F
        md, re_ = c["max_dropout"], c["reach"]
        for kw in (dict(max_dropout=min(md + 1, pi.NO_LIMIT)), dict(max_dropout=pi.NO_LIMIT), dict(reach=min(re_ + 1, 65535)), dict(reach=65535)):
            assert (model(c, **kw)["run"] >= got["run"]).all(), (seed, kw)
        # G
        for sl, one in pi.single_streams(c):
            alone = model(one)
            for k in ("flags", "run", "pos"):
                assert np.array_equal(alone[k], got[k][sl]), (seed, k)


def test_random_draws_cover_their_ranges():
    cs = [pi.random_case(s) for s in range(200)]
    lens = np.concatenate([np.diff(c["soff"].astype(np.int64)) for c in cs])
    assert lens.min() == 0 and 290 <= lens.max() <= 300
    assert any(c["box"] is None for c in cs) and any(c["box"] is not None for c in cs)
    assert any(c["sd"] is None for c in cs) and any(c["sd"] is not None for c in cs)
    bx = np.concatenate([c["box"] for c in cs if c["box"] is not None])
    none = (bx["x0"] == 0xFFFF) & (bx["y0"] == 0xFFFF) & (bx["x1"] == 0xFFFF) & (bx["y1"] == 0xFFFF)
    assert none.any() and (bx["x1"][~none] < pi.GRID_W).all() and (bx["y1"][~none] < pi.GRID_H).all()
    assert {2, 255} <= set(np.concatenate([c["flags"] for c in cs]).tolist())
    # the link rule bites both ways somewhere
    linked = [pm.persist(c["flags"], c["soff"], c["sd"], c["box"], max_dropout=pi.NO_LIMIT, reach=c["reach"])["run"] for c in cs if c["box"] is not None]
    assert any((r > 1).any() for r in linked) and any((r == 1).any() for r in linked)


# ------------------------------------------------------------------ the GPU tier's generated batches are what they claim

def test_seam_cases_sit_on_their_seams():
    plan = m.persist_preview()
    T, wg = plan["frames_per_tile"], plan["workgroup"]
    cases = pi.seam_cases(T, wg)
    assert all(len(c["flags"]) == 3 * T + 5 and len(c["soff"]) == 2 for c in cases.values())
    for k in pi.seam_positions(T, wg):
        got = model(cases[f"start@{k}"])
        assert got["pos"][k] == 1 and got["run"][k] == 7 and got["run"][k - 3] == 8
        got = model(cases[f"end@{k}"])
        assert got["pos"][k - 1] == got["run"][k - 1] == 9 and got["flags"][k] == 0 and got["pos"][k + 3] == 1
        for md in (0, 1, 5):
            c = cases[f"streak{md}/{md}@{k}"]
            assert int((c["flags"] != 0).sum()) == 12 and (model(c)["run"][c["flags"] != 0] == 12).all()             # bridged
            c = cases[f"streak{md + 1}/{md}@{k}"]
            assert (model(c)["run"][c["flags"] != 0] == 6).all()                                                      # one too many
            assert c["flags"][k] == 0 and (md == 0 or c["flags"][k - 1] == 0)                                         # across the seam
        for quiet in "TQ":
            assert model(cases[f"tile-back-{quiet}-linked@{k}"])["run"][[k, k + T]].tolist() == [2, 2]
            assert model(cases[f"tile-back-{quiet}-apart@{k}"])["run"][[k, k + T]].tolist() == [1, 1]
    n = 3 * T + 5
    assert model(cases["whole-stream-run"])["run"][[0, n - 1]].tolist() == [2, 2]
    assert (model(cases["all-M"])["run"] == n).all() and model(cases["all-M"])["pos"].tolist() == list(range(1, n + 1))
    assert not model(cases["all-Q"])["run"].any() and not model(cases["all-T"])["run"].any()


def test_shapes_case_has_the_listed_streams():
    plan = m.persist_preview()
    T = plan["frames_per_tile"]
    lens = pi.shape_lengths(T)
    assert lens[:8] == [0, 1, 2, 64, T, T + 1, 0, 0] and len(lens) == 72 and set(lens[8:]) == {1, 2, 3}
    c = pi.shapes_case(T)
    assert int(c["soff"][0]) == 3 and len(c["flags"]) == int(c["soff"][-1]) + 5
    assert np.diff(c["soff"].astype(np.int64)).tolist() == lens
    got = model(c)
    outside = np.r_[0:3, int(c["soff"][-1]):len(c["flags"])]
    assert (c["flags"][outside] != 0).all() and not any(got[k][outside].any() for k in got)


def test_example_stream_gives_the_examples_counts():
    fl, sd = pi.example_flags()
    got = pm.persist(fl, [0, len(fl)], sd, None, min_run=3)
    assert int((fl != 0).sum()) == 36 and int(got["flags"].sum()) == 29 and int(got["run"].max()) == 29
    assert np.flatnonzero(got["flags"]).tolist() == [f for f in range(121, 150)]
    src = open(os.path.join(ROOT, "examples", "persist_example.c")).read()
    assert "motion[0] != 36" in src and "motion[1] != 29" in src


# ------------------------------------------------------------------ the command's options

def test_persist_command_usage_errors(capsys):
    for args in ([], ["x.mtmv", "--min-run", "0"], ["x.mtmv", "--min-run", "2,2"], ["x.mtmv", "--min-run", "a"],
                 ["x.mtmv", "--min-run", ",".join(str(i) for i in range(1, 18))], ["x.mtmv", "--max-dropout", "-1"],
                 ["x.mtmv", "--max-dropout", "4294967296"], ["x.mtmv", "--reach", "2"], ["x.mtmv", "--min-blob-cells", "4"],
                 ["x.mtmv", "--blobs", "--reach", "65536"], ["x.mtmv", "--blobs", "--reach", "-1"], ["x.mtmv", "--blobs", "--min-blob-cells", "0"]):
        with pytest.raises(SystemExit) as ei:
            persist.main(args)
        assert ei.value.code == 2, args
        assert "usage" in capsys.readouterr().err
    ns = persist.parser().parse_args(["x.mtmv"])
    assert ns.min_run == [1, 2, 3, 5] and ns.max_dropout == 0 and not ns.blobs and ns.reach is None and ns.min_blob_cells is None
    ns = persist.parser().parse_args(["x.mtmv", "--blobs", "--reach", "3", "--min-blob-cells", "4", "--min-run", "3,7", "--max-dropout", "4294967295",
                                      "--keep", "k.mtkeep", "--json", "--width", "1920", "--max-gap-sec", "2.5"])
    assert (ns.blobs, ns.reach, ns.min_blob_cells, ns.min_run, ns.max_dropout, ns.keep, ns.json) == (True, 3, 4, [3, 7], 0xFFFFFFFF, "k.mtkeep", True)
    assert persist.levels_with_one([3, 7]) == [1, 3, 7] and persist.levels_with_one([2, 1]) == [2, 1]
    assert persist.main(["/nonexistent/x.mtmv"]) == 1 and "cannot read" in capsys.readouterr().err
    run = np.array([1, 0, 3, 3, 3, 0, 12, 0], dtype=np.uint32)
    pos = np.array([1, 0, 1, 2, 3, 0, 1, 0], dtype=np.uint32)
    assert persist.histogram(run, pos) == {"1": 1, "2": 0, "3-4": 1, "5-9": 0, "10-29": 1, "30-99": 0, "100+": 0}
