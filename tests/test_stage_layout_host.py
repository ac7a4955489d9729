"""CPU tier: the block layout of the host forms' staging (mtgpu::stage_layout, csrc/api_common.h) in a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/stage_layout_check.cpp holds it to the formulas the host
forms wrote out by hand before, on a few thousand random combinations of present and absent inputs and outputs."""
import os
import subprocess

import mvtrim_amd as m

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(m.LIB_PATH)


def test_stage_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_layout_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(HERE, "cpp", "stage_layout_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "4000", "23"], capture_output=True, text=True,
                         env={"PATH": os.environ.get("PATH", ""), "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok 16000 layouts"
