"""CPU tier: the setting sweep (include/mtgpu_sweep.h) exists at every layer — header, library, ctypes table, Python
package, command — plans its passes with host arithmetic alone, rejects bad arguments before any HIP call, and has no
fallback without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, tune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_scan_frames_sweep", "mtgpu_scan_sweep_device", "mtgpu_scan_sweep_preview"]


def sweep_header():
    return open(os.path.join(ROOT, "include", "mtgpu_sweep.h")).read()


def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = sweep_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_SWEEP)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_SWEEP[n][1], n
        # every declaration names the reference lines it stands for
        at = hdr.index("int " + n + "(")
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert "#define MT_SWEEP_MAX_THRESHOLDS 8" in hdr and "#define MT_SWEEP_MAX_VECTORS 8" in hdr
    assert (_abi.SWEEP_MAX_THRESHOLDS, _abi.SWEEP_MAX_VECTORS) == (8, 8) and C.sizeof(_abi.SweepPlanC) == 16
    # mtgpu.h hands the declarations to everyone who includes it
    assert '#include "mtgpu_sweep.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # the kernels are in the library, and nothing of the checker is
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"sweep_frames_kernel" in blob and b"sweep_clear_kernel" in blob
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    assert "mto_" not in syms


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_sweep_plan p;\n"
            "  return mtgpu_scan_sweep_preview(0, 163840, MT_SWEEP_MAX_THRESHOLDS, MT_SWEEP_MAX_VECTORS, &p)\n"
            "       + mtgpu_scan_sweep_device(c, 0, 40, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0)\n"
            "       + mtgpu_scan_frames_sweep(c, 0, 0, 0, 0, 0, 1, 0, 1, 0) + p.passes + p.thresholds_per_pass + p.lds_bytes\n"
            "       + p.counter_bits;\n}\n")
    for first in ("mtgpu.h", "mtgpu_sweep.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def preview(params, n_thr, n_vec, lds=MI355X_LDS):
    p = _abi.SweepPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_scan_sweep_preview(C.byref(c), lds, n_thr, n_vec, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def test_preview_plans_the_passes():
    hd = m.ScanParams.from_config(1920, 1080)
    uhd = m.ScanParams.from_config(3840, 2160)
    for n_vec in (1, 4, 8):
        rc, p, _ = preview(hd, 4, n_vec)
        assert rc == _abi.MT_OK and p.passes == 1 and p.thresholds_per_pass == 4 and p.counter_bits == 32
        assert 4 * 64 * 120 * 4 < p.lds_bytes <= MI355X_LDS            # four tiles of (62 + 2) x 120 counters, and masks
        rc, p, _ = preview(hd, 8, n_vec)
        assert rc == _abi.MT_OK and p.passes <= 2 and p.thresholds_per_pass * p.passes >= 8
        rc, p, _ = preview(uhd, 2, n_vec)
        assert rc == _abi.MT_OK and p.passes <= 2 and p.thresholds_per_pass * p.passes >= 2
        assert 125 * 240 * 4 < p.lds_bytes <= MI355X_LDS
    # the grids the plain scan cuts into row bands have no sweep form
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2), 1, 1)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0), 1, 1)
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    # counts outside [1, 8]
    for n_thr, n_vec, name in ((0, 1, "n_thresholds"), (9, 1, "n_thresholds"), (1, 0, "n_vectors"), (1, 9, "n_vectors")):
        rc, _, msg = preview(hd, n_thr, n_vec)
        assert rc == _abi.MT_ERR_INVALID and name in msg
    assert m.load_library().mtgpu_scan_sweep_preview(None, MI355X_LDS, 1, 1, C.byref(_abi.SweepPlanC())) == _abi.MT_ERR_INVALID
    c = hd.to_c()
    assert m.load_library().mtgpu_scan_sweep_preview(C.byref(c), MI355X_LDS, 1, 1, None) == _abi.MT_ERR_INVALID
    # thresholds_per_pass x passes >= T always, on whatever fits: every grid of the edge sets, every count, three LDS sizes
    for (w, h, kw) in [(1920, 1080, {}), (3840, 2160, {}), (1280, 720, {}), (640, 480, {}), (16, 16, dict(vertical_mask=0.0)),
                       (2064, 96, {}), (1920, 1080, dict(block_size=8, block_shift=3)), (1920, 1080, dict(vertical_mask=0.5))]:
        params = m.ScanParams.from_config(w, h, **kw)
        for lds in (65536, 98304, MI355X_LDS):
            for n_thr in range(1, 9):
                for n_vec in (1, 8):
                    rc, p, msg = preview(params, n_thr, n_vec, lds)
                    if rc == _abi.MT_ERR_UNSUPPORTED:
                        continue
                    assert rc == _abi.MT_OK, msg
                    assert p.thresholds_per_pass * p.passes >= n_thr and p.passes >= 1 and p.thresholds_per_pass >= 1
                    assert (p.passes - 1) * p.thresholds_per_pass < n_thr and 0 < p.lds_bytes <= lds
    assert m.sweep_preview(hd, 4, 4) == {"thresholds_per_pass": 4, "passes": 1, "lds_bytes": preview(hd, 4, 4)[1].lds_bytes,
                                         "counter_bits": 32}


def test_invalid_arguments_are_rejected_without_a_device():
    """Every check that needs no device runs before the first HIP call."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(8)           # never dereferenced: the context is what is wrong
    thr, vec = (C.c_double * 1)(4.0), (C.c_int32 * 1)(2)
    assert lib.mtgpu_scan_sweep_device(None, one, 40, 1, one, None, 1, thr, 1, vec, 1, one, None) == inv
    assert b"ctx" in lib.mtgpu_last_error()
    out = np.full(3, 7, dtype=np.uint32)
    off = np.array([0, 0], dtype=np.uint64)
    assert lib.mtgpu_scan_frames_sweep(None, None, off.ctypes.data_as(C.c_void_p), None, 1, thr, 1, vec, 1,
                                       out.ctypes.data_as(C.c_void_p)) == inv
    assert b"ctx" in lib.mtgpu_last_error() and out.tolist() == [7, 7, 7]


def test_package_exports_the_methods():
    for name in ("sweep_centres", "sweep_centres_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.sweep_preview) and callable(tune.main) and callable(tune.load) and callable(tune.study)


# ------------------------------------------------------------------ the command's arguments

GOOD = ["--mv-threshold-sq", "1,4,16", "--vectors-needed", "1,2,4", "--clusters-needed", "1,2,4"]


def test_tune_lists_parse():
    a = tune.parser().parse_args(["f.mtmv"] + GOOD + ["--json"])
    assert a.mv_threshold_sq == [1.0, 4.0, 16.0] and a.vectors_needed == [1, 2, 4] and a.clusters_needed == [1, 2, 4]
    assert a.json and a.file == "f.mtmv" and a.width is None and a.max_gap_sec is None
    a = tune.parser().parse_args(["f", "--mv-threshold-sq", "24.5, 25,inf,nan,-1", "--vectors-needed", "0,259,255",
                                  "--clusters-needed", "0", "--width", "1920", "--height", "1080", "--duration", "3.5"])
    assert a.mv_threshold_sq[:3] == [24.5, 25.0, float("inf")] and np.isnan(a.mv_threshold_sq[3]) and a.mv_threshold_sq[4] == -1.0
    assert a.vectors_needed == [0, 259, 255] and a.clusters_needed == [0] and (a.width, a.height, a.duration) == (1920, 1080, 3.5)


@pytest.mark.parametrize("bad", [
    ["--mv-threshold-sq", "1,,4"], ["--mv-threshold-sq", "1,x"], ["--mv-threshold-sq", ""],
    ["--mv-threshold-sq", "1,2,3,4,5,6,7,8,9"], ["--vectors-needed", "1.5"], ["--vectors-needed", "1,2,3,4,5,6,7,8,9"],
    ["--vectors-needed", "4294967296"], ["--clusters-needed", "a"], ["--clusters-needed", ",".join(["1"] * 17)],
])
def test_tune_bad_lists_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    """argparse's exit code 2, and neither the file nor a scanner has been looked at."""
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(tune, "MotionScanner", boom)
    monkeypatch.setattr(tune, "load", boom)
    monkeypatch.setattr(tune.ScanParams, "from_config", boom)
    args = list(GOOD)
    args[args.index(bad[0]) + 1] = bad[1]
    with pytest.raises(SystemExit) as ei:
        tune.main(["nothing_here.mtmv"] + args)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_tune_missing_option_and_missing_geometry_exit_2(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(tune, "MotionScanner", boom)
    with pytest.raises(SystemExit) as ei:
        tune.main(["f.mtmv", "--mv-threshold-sq", "1", "--vectors-needed", "1"])
    assert ei.value.code == 2
    # a JSON carries no width / height / duration
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])
    with pytest.raises(SystemExit) as ei:
        tune.main([path] + GOOD)
    assert ei.value.code == 2
    assert tune.main([str(tmp_path / "nothing_here.json")] + GOOD) == 1


def test_tune_has_no_fallback_without_a_device(tmp_path):
    """A readable file: rows with a device, a non-zero exit and no rows without one — never numbers from somewhere
    else."""
    mv = np.zeros(4, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"], mv["src_x"], mv["src_y"] = [40, 41, 56, 57], 40, [30, 31, 46, 47], 40
    path = str(tmp_path / "two.mtmv")
    m.mvfile.write_mtmv(path, 160, 160, 1, 1000, 25.0, 1.0, [0, 40], [mv, None])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.tune", path, "--mv-threshold-sq", "4", "--vectors-needed", "2",
                          "--clusters-needed", "1,3", "--json"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    if m.load_library().mtgpu_device_count() > 0:
        # cells (2, 2) and (3, 2) of a 10 x 10 grid hold two votes each: 2 centres
        import json
        assert out.returncode == 0, out.stderr
        rows = json.loads(out.stdout)["rows"]
        assert [(r["clusters_needed"], r["motion_frames"]) for r in rows] == [(1, 1), (3, 0)]
        return
    assert out.returncode != 0 and out.stdout == ""
    assert "no CPU fallback" in out.stderr
