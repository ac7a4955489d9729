"""CPU tier: the activity maps (include/mtgpu_activity.h) exist at every layer — header, library, ctypes table, Python
package, command — choose their LDS form with host arithmetic alone, reject bad arguments before any HIP call, and
have no fallback without a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, activity, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MI355X_LDS = 163840

NEW_SYMBOLS = ["mtgpu_activity_map", "mtgpu_activity_map_device", "mtgpu_activity_preview"]


def activity_header():
    return open(os.path.join(ROOT, "include", "mtgpu_activity.h")).read()


def test_entry_points_are_declared_exported_and_prototyped():
    lib = m.load_library()
    hdr = activity_header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_ACTIVITY)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_ACTIVITY[n][1], n
        assert n not in _abi.ABI                  # mtgpu.h's own text does not declare it
        # every declaration names the reference lines it stands for
        at = hdr.index("int " + n + "(")
        assert "src/motion_scanner.cpp:" in hdr[hdr.rindex("\n/*", 0, at):at], n
    assert C.sizeof(_abi.ActivityPlanC) == 16
    assert [f for f, _ in _abi.ActivityPlanC._fields_] == ["lds_bytes", "acc_bits", "max_run", "workgroup"]
    # mtgpu.h hands the declarations to everyone who includes it
    assert '#include "mtgpu_activity.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # no new environment variable
    assert "getenv" not in open(os.path.join(ROOT, "motion-estimated-video-trimmer_amd", "csrc", "activity_kernels.hip")).read()
    # the kernels are in the library, and nothing of the checker is
    blob = open(_abi.LIB_PATH, "rb").read()
    assert b"activity_frames_kernel" in blob and b"activity_clear_kernel" in blob
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _abi.LIB_PATH]).decode()
    assert "mto_" not in syms


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = ("int use(mtgpu_ctx *c) {\n"
            "  mtgpu_activity_plan p;\n"
            "  return mtgpu_activity_preview(0, 163840, &p)\n"
            "       + mtgpu_activity_map_device(c, 0, 40, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0)\n"
            "       + mtgpu_activity_map(c, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0) + p.lds_bytes + p.acc_bits + p.max_run + p.workgroup;\n}\n")
    for first in ("mtgpu.h", "mtgpu_activity.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def preview(params, lds=MI355X_LDS):
    p = _abi.ActivityPlanC()
    c = params.to_c()
    rc = m.load_library().mtgpu_activity_preview(C.byref(c), lds, C.byref(p))
    return rc, p, m.load_library().mtgpu_last_error().decode()


def test_preview_chooses_the_form():
    # 1080p, code defaults and shipped env: LDS accumulators
    for kw in (config.CODE_DEFAULTS, config.SHIPPED_ENV):
        rc, p, msg = preview(m.ScanParams.from_config(1920, 1080, **kw))
        assert rc == _abi.MT_OK, msg
        assert p.acc_bits in (16, 32) and p.max_run >= 1 and p.workgroup > 0 and p.workgroup % 64 == 0
        # tile of (62 + 2) x 120 counters, two planes of 62 x 120 fields
        assert 64 * 120 * 4 + 2 * 62 * 120 * p.acc_bits // 8 < p.lds_bytes <= MI355X_LDS
        if p.acc_bits == 16:
            assert p.max_run <= 65535
    # 4K defaults: a 125 x 240 x 4 B tile leaves no room for two planes of 123 x 240 fields
    rc, p, msg = preview(m.ScanParams.from_config(3840, 2160, **config.CODE_DEFAULTS))
    assert rc == _abi.MT_OK, msg
    assert p.acc_bits == 0 and p.max_run == 1 and 125 * 240 * 4 < p.lds_bytes <= MI355X_LDS
    # the grids the plain scan cuts into row bands have no form
    rc, _, msg = preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "960x540" in msg
    rc, _, msg = preview(m.ScanParams.from_config(32767, 3, block_size=1, block_shift=0, vertical_mask=0.0))
    assert rc == _abi.MT_ERR_UNSUPPORTED and "32767x3" in msg
    # invalid
    lib = m.load_library()
    hd = m.ScanParams.from_config(1920, 1080)
    assert lib.mtgpu_activity_preview(None, MI355X_LDS, C.byref(_abi.ActivityPlanC())) == _abi.MT_ERR_INVALID
    c = hd.to_c()
    assert lib.mtgpu_activity_preview(C.byref(c), MI355X_LDS, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_activity_preview(C.byref(c), 100, C.byref(_abi.ActivityPlanC())) == _abi.MT_ERR_INVALID
    # whatever fits: lds_bytes within the budget, a 16-bit plan never lets a field wrap, no accumulators -> every frame flushes
    seen = set()
    for (w, h, kw) in [(1920, 1080, {}), (3840, 2160, {}), (1280, 720, {}), (640, 480, {}), (16, 16, dict(vertical_mask=0.0)),
                       (2064, 96, {}), (1920, 1080, dict(block_size=8, block_shift=3)), (1920, 1080, dict(vertical_mask=0.5)),
                       (3840, 2160, dict(vertical_mask=0.0)), (3840, 2160, dict(vertical_mask=0.3))]:
        params = m.ScanParams.from_config(w, h, **kw)
        for lds in (65536, 98304, MI355X_LDS):
            rc, p, msg = preview(params, lds)
            if rc == _abi.MT_ERR_UNSUPPORTED:
                continue
            assert rc == _abi.MT_OK, msg
            assert 0 < p.lds_bytes <= lds and p.acc_bits in (0, 16, 32) and p.max_run >= 1 and p.workgroup == 1024
            assert p.acc_bits != 16 or p.max_run <= 65535
            assert p.acc_bits != 0 or p.max_run == 1
            seen.add(p.acc_bits)
    assert seen == {0, 16, 32}
    got = m.activity_preview(hd)
    assert got == {"lds_bytes": preview(hd)[1].lds_bytes, "acc_bits": preview(hd)[1].acc_bits,
                   "max_run": preview(hd)[1].max_run, "workgroup": 1024}
    with pytest.raises(m.MtgpuError) as ei:
        m.activity_preview(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED


def test_invalid_arguments_are_rejected_without_a_device():
    """Every check that needs no device runs before the first HIP call."""
    lib = m.load_library()
    inv = _abi.MT_ERR_INVALID
    one = C.c_void_p(8)           # never dereferenced: the context is what is wrong
    assert lib.mtgpu_activity_map_device(None, one, 40, 1, one, None, 1, one, 1, 0, 0, one, one, one, None) == inv
    assert b"ctx" in lib.mtgpu_last_error()
    out = np.full(3, 7, dtype=np.uint32)
    off = np.array([0, 0], dtype=np.uint64)
    soff = np.array([0, 1], dtype=np.uint64)
    assert lib.mtgpu_activity_map(None, None, off.ctypes.data_as(C.c_void_p), None, 1, soff.ctypes.data_as(C.c_void_p), 1, 0,
                                  out.ctypes.data_as(C.c_void_p), None, None) == inv
    assert b"ctx" in lib.mtgpu_last_error() and out.tolist() == [7, 7, 7]


def test_package_exports_the_methods():
    for name in ("activity_map", "activity_map_device"):
        assert callable(getattr(m.MotionScanner, name)), name
    assert callable(m.activity_preview) and "activity_preview" in m.__all__
    assert callable(activity.main) and callable(activity.measure) and callable(activity.row_table) and callable(activity.mask_table)
    with pytest.raises(ValueError):
        m.MotionScanner.activity_map(None, None, None, want=("active", "heat"))


def test_gpu_test_inputs_hold_centres_to_count():
    """Checked once on the CPU (as tests/test_scan_inputs.py does for the scan): the inputs of tests/test_gpu_activity.py
    have centres and active cells to count in every stream set, the model agrees with the oracle on them, and
    min_centres separates frames.  A parity test on all-zero maps shows nothing."""
    import test_gpu_activity as ga
    for which in (0, 1):
        _, (active, centre, frames, counts) = ga.parity_model(which, 0)         # asserts the oracle identities itself
        assert int(centre.sum()) > 100 and int(active.sum()) > int(centre.sum())
        assert frames.tolist()[1:] == [int(x) for x in frames[1:]] and int(frames[1]) > 20 and int(frames[2]) > 50
        assert int(active[:, :3].sum()) == 0 and int(active[:, 65:].sum()) == 0  # masked rows
        assert int(active[:, :, 0].sum()) + int(active[:, :, 119].sum()) > 0     # edge columns: active, never centres
        assert int(centre[:, :, 0].sum()) + int(centre[:, :, 119].sum()) == 0
        assert int((active > 1).sum()) > 0                                       # cells that several frames add to
    c1 = [int(ga.parity_model(1, k)[1][2].sum()) for k in (0, 1, 2, 10 ** 9)]
    assert c1[0] > c1[1] >= c1[2] > c1[3] == 0
    p, many, one = ga.boundary_model()
    assert int(many[1].sum()) == int(one[1].sum()) > 4000 and int(one[2][0]) == int(many[2].sum()) > 3500
    assert int(one[0].max()) > 1 and int((many[2] == 7).sum()) > 0 and int((many[2] < 7).sum()) > 0


# ------------------------------------------------------------------ the command's arguments

def test_activity_lists_parse():
    a = activity.parser().parse_args(["f.mtmv", "--vertical-mask", "0,0.05, 0.1", "--json", "--npy", "out/p"])
    assert a.vertical_mask == [0.0, 0.05, 0.1] and a.json and a.npy == "out/p" and a.min_centres == 0 and not a.kept
    a = activity.parser().parse_args(["f", "--min-centres", "3", "--width", "1920", "--height", "1080", "--vectors-needed", "4",
                                      "--block-shift", "4", "--mv-threshold-sq", "4"])
    assert a.min_centres == 3 and a.vertical_mask is None and (a.width, a.height) == (1920, 1080)
    assert (a.vectors_needed, a.block_shift, a.mv_threshold_sq) == (4, 4, 4.0)
    assert activity.parser().parse_args(["f", "--kept"]).kept
    assert "estimate" in activity.parser().format_help().lower() and "not the count a masked scan returns" in \
        " ".join(activity.parser().format_help().split())


@pytest.mark.parametrize("bad", [
    ["--vertical-mask", "0,,0.1"], ["--vertical-mask", "0,x"], ["--vertical-mask", ""], ["--vertical-mask", "nan"],
    ["--vertical-mask", "-0.1"], ["--vertical-mask", "inf"], ["--vertical-mask", ",".join(["0.1"] * 17)],
    ["--min-centres", "-1"], ["--min-centres", "1.5"], ["--min-centres", "4294967296"],
    ["--min-centres", "2", "--kept"],
])
def test_activity_bad_lists_exit_2_before_any_device_is_touched(bad, monkeypatch, capsys):
    """argparse's exit code 2, and neither the file nor a scanner has been looked at."""
    def boom(*a, **k):
        raise AssertionError("touched before the arguments were valid")
    monkeypatch.setattr(activity, "MotionScanner", boom)
    monkeypatch.setattr(activity.tune, "load", boom)
    monkeypatch.setattr(activity.ScanParams, "from_config", boom)
    with pytest.raises(SystemExit) as ei:
        activity.main(["nothing_here.mtmv"] + bad)
    assert ei.value.code == 2 and bad[0] in capsys.readouterr().err


def test_activity_missing_geometry_exits_2_and_missing_file_1(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a scanner was created before the arguments were valid")
    monkeypatch.setattr(activity, "MotionScanner", boom)
    mv = np.zeros(1, dtype=m.MV_DTYPE)
    path = str(tmp_path / "one.json")
    m.mvjson.write_json(path, [mv], [0.0])           # a JSON carries no width / height
    with pytest.raises(SystemExit) as ei:
        activity.main([path])
    assert ei.value.code == 2
    assert activity.main([str(tmp_path / "nothing_here.json")]) == 1


def test_tables_from_a_map():
    """The two tables are plain sums over the map (no device)."""
    centre = np.zeros((10, 4), dtype=np.uint32)
    active = np.zeros((10, 4), dtype=np.uint32)
    centre[0, 1], centre[4, 2], centre[9, 1] = 1, 6, 1
    active[0], active[4] = 2, 3
    rows = activity.row_table(active, centre)
    assert [(r["active"], r["centre"]) for r in rows][:5] == [(8, 1), (0, 0), (0, 0), (0, 0), (12, 6)]
    assert rows[4]["centre_share"] == 0.75 and sum(r["centre_share"] for r in rows) == 1.0
    t = activity.mask_table(centre, [(0.0, 0), (0.1, 1), (0.6, 6)])
    assert [r["centre_share_dropped"] for r in t] == [0.0, 0.25, 1.0] and [r["margin_rows"] for r in t] == [0, 1, 6]
    assert all("estimate" in r["kind"] for r in t)
    assert activity.mask_table(np.zeros((4, 4), dtype=np.uint32), [(0.1, 0)])[0]["centre_share_dropped"] == 0.0


def test_activity_has_no_fallback_without_a_device(tmp_path):
    """A readable file: the table with a device, a non-zero exit and no rows without one — never numbers from somewhere
    else."""
    mv = np.zeros(4, dtype=m.MV_DTYPE)
    mv["dst_x"], mv["dst_y"], mv["src_x"], mv["src_y"] = [40, 41, 56, 57], 40, [30, 31, 46, 47], 40
    path = str(tmp_path / "two.mtmv")
    m.mvfile.write_mtmv(path, 160, 160, 1, 1000, 25.0, 1.0, [0, 40], [mv, None])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "mvtrim_amd.activity", path, "--mv-threshold-sq", "4", "--vectors-needed", "2",
                          "--json"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    if m.load_library().mtgpu_device_count() > 0:
        # cells (2, 2) and (3, 2) of a 10 x 10 grid hold two votes each: both active, both centres, in one frame
        import json
        assert out.returncode == 0, out.stderr
        doc = json.loads(out.stdout)
        assert doc["contributing_frames"] == 1 and [(r["active"], r["centre"]) for r in doc["rows"]][2] == (2, 2)
        return
    assert out.returncode != 0 and out.stdout == ""
    assert "no CPU fallback" in out.stderr


def test_plain_c_example_compiles_and_links(tmp_path):
    """examples/activity_example.c against the header and the library as they are (it runs in the GPU tier)."""
    pkg = os.path.dirname(m.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "activity_example.c"), "-o", str(tmp_path / "activity_example"),
                           "-L" + pkg, "-lmtgpu", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
