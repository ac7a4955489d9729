"""CPU tier: the motion-scalar entry points (tools/motion_scalar.cpp:61-84 on the GPU) exist at every layer — header,
library, ctypes table, Python package, command — reject bad arguments before any HIP call, and have no fallback
without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["mtgpu_motion_bins_device", "mtgpu_motion_scalar", "mtgpu_motion_scores_device"]


def motion_header():
    return open(os.path.join(ROOT, "include", "mtgpu_motion.h")).read()


def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = motion_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_MOTION)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_MOTION[n][1], n
        # every declaration names the reference lines it replaces
        at = hdr.index("int " + n + "(")
        assert "tools/motion_scalar.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    # mtgpu.h hands the declarations to everyone who includes it
    assert '#include "mtgpu_motion.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # the kernels are in the library, and nothing of the checker is
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"motion_scores_kernel" in blob and b"motion_bins_kernel" in blob
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    assert "mto_" not in syms


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  return mtgpu_motion_scores_device(c, 0, 0, 0, 0, 0, 0, 0) + mtgpu_motion_bins_device(c, 0, 0, 0, 0, 0, 1, 0, 0, 0)\n"
            "       + mtgpu_motion_scalar(c, 0, 0, 0, 0, 1, 0, 0);\n}\n")
    for first in ("mtgpu.h", "mtgpu_motion.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_invalid_arguments_are_rejected_without_a_device():
    """Every check that needs no device runs before the first HIP call: NULL context, NULL required pointers,
    n_sec == 0."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(8)           # never dereferenced: the context is what is wrong
    assert lib.mtgpu_motion_scores_device(None, one, 1, one, 1, one, one, None) == inv
    assert b"ctx" in lib.mtgpu_last_error()
    assert lib.mtgpu_motion_bins_device(None, one, one, one, one, 1, 1, one, one, None) == inv
    assert b"ctx" in lib.mtgpu_last_error()
    assert lib.mtgpu_motion_scalar(None, one, one, one, 1, 1, one, one) == inv
    assert b"ctx" in lib.mtgpu_last_error()
    # a context that could not be created stays NULL: still MT_ERR_INVALID, nothing is written
    off = np.array([0, 0], dtype=np.uint64)
    pts = np.zeros(1)
    acc = np.full(3, 7.0)
    assert lib.mtgpu_motion_scalar(None, None, off.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p), 1, 3,
                                   acc.ctypes.data_as(C.c_void_p), None) == inv
    assert acc.tolist() == [7.0, 7.0, 7.0]


def test_package_exports_the_methods():
    for name in ("motion_scores", "motion_scores_device", "motion_bins_device", "motion_scalar"):
        assert callable(getattr(m.MotionScanner, name)), name
    from mvtrim_amd import motion_scalar as cmd
    assert callable(cmd.main) and callable(cmd.load)


def test_motion_scalar_has_no_fallback_without_a_device():
    """Without a device the path fails as check_frames does: MT_ERR_DEVICE from the library, nothing computed on the
    CPU.  (With a device: the smallest known answer — one 3-4-5 vector on an 8x8 block in second 2.)"""
    lib = m.load_library()
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    mv["motion_x"], mv["motion_y"], mv["motion_scale"], mv["w"], mv["h"] = 12, 16, 4, 8, 8
    batch = m.FrameBatch.from_frames([mv])
    params = m.ScanParams.from_config(160, 160)
    if lib.mtgpu_device_count() > 0:
        with m.MotionScanner(params) as s:
            acc, bt = s.motion_scalar(batch, [2.5])
        assert acc.tolist() == [0.0, 0.0, 320.0] and bt.tolist() == [0, 0, 1]
        return
    with pytest.raises(m.MtgpuError) as ei:
        with m.MotionScanner(params) as s:
            s.motion_scalar(batch, [2.5])
    assert ei.value.code == _abi.MT_ERR_DEVICE and "no CPU fallback" in str(ei.value)


def run_command(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "mvtrim_amd.motion_scalar"] + args, capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=120)


def test_command_refuses_a_missing_file(tmp_path):
    out = run_command([str(tmp_path / "nothing_here.json")])
    assert out.returncode != 0 and out.stdout == ""
    assert "cannot read" in out.stderr
    bad = tmp_path / "bad.json"
    bad.write_text("{ not json")
    out = run_command([str(bad)])
    assert out.returncode != 0 and out.stdout == ""


def test_command_without_a_device_fails_loudly(tmp_path):
    """A readable file but no device: a non-zero exit and no CSV, never numbers from somewhere else."""
    if m.load_library().mtgpu_device_count() > 0:
        pytest.skip("a GPU is present; the no-device failure path is for the CPU tier")
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    mv["motion_x"], mv["motion_scale"], mv["w"], mv["h"] = 4, 1, 2, 2
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])
    out = run_command([path])
    assert out.returncode != 0 and "second,motion_value" not in out.stdout
    assert "no CPU fallback" in out.stderr
