"""CPU tier: the keep mask of a pipe (include/mtgpu_pipe_zones.h) exists at every layer — header, library, ctypes table,
ScanPipe, the C++ host layer, mtgpu_scan_file — and answers bad calls before any HIP call; the `.mtkeep` text format
round-trips between Python and the C++ parser and every malformed file is refused with its line; and the inputs of
tests/test_gpu_pipe_zones.py do, by the oracle on filtered records, what the GPU cases need them to do."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi, zones

import pipe_zones_inputs as pz
import zones_inputs as zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.dirname(m.LIB_PATH)
NEW_SYMBOLS = ["mtgpu_pipe_has_keep", "mtgpu_pipe_set_keep"]


def header():
    return open(os.path.join(ROOT, "include", "mtgpu_pipe_zones.h")).read()


# ------------------------------------------------------------------ exports and early errors

def test_entry_points_are_declared_exported_and_refuse_a_null_pipe():
    lib = m.load_library()
    hdr = header()
    declared = sorted(set(re.findall(r"\b(mtgpu_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == NEW_SYMBOLS == sorted(_abi.ABI_PIPE_ZONES)
    for n in NEW_SYMBOLS:
        fn = getattr(lib, n)                      # AttributeError: not exported by libmtgpu.so
        assert fn.restype is C.c_int and fn.argtypes == _abi.ABI_PIPE_ZONES[n][1], n
        # every declaration cites the reference lines it stands for: the active-cell test and the check_frame call site
        at = hdr.index("int " + n + "(")
        comment = hdr[hdr.rindex("\n/*", 0, at):at]
        assert "src/motion_scanner.cpp:282" in comment and ":375-383" in comment, n
    assert '#include "mtgpu_pipe_zones.h"' in open(os.path.join(ROOT, "include", "mtgpu.h")).read()
    # a NULL pipe: answered from the arguments alone, no device needed
    words = np.zeros(68 * 2, dtype=np.uint64)
    assert lib.mtgpu_pipe_set_keep(None, words.ctypes.data_as(C.c_void_p)) == _abi.MT_ERR_INVALID
    assert "NULL" in lib.mtgpu_last_error().decode()
    assert lib.mtgpu_pipe_set_keep(None, None) == _abi.MT_ERR_INVALID
    assert lib.mtgpu_pipe_has_keep(None) == -1
    # no new layout bit, no new environment variable
    assert (m.LAYOUT_AOS40 | m.LAYOUT_ZERO_COPY | m.LAYOUT_CENTRES) == 7
    zones_src = open(os.path.join(PKG, "csrc", "zones_kernels.hip")).read()
    assert "getenv" not in zones_src
    pipe_src = open(os.path.join(PKG, "csrc", "pipe.hip")).read()
    parent_env = {"MTGPU_INJECT_SUBMIT_FAIL", "MTGPU_INJECT_GROW_FAIL", "MTGPU_INJECT_COLLECT_FAIL", "MTGPU_INJECT_ONCE"}
    assert set(re.findall(r'getenv\("([A-Z_]+)"\)', pipe_src)) == parent_env
    # the pipe form of the kernel is in the library: both record layouts
    blob = open(_abi.LIB_PATH, "rb").read()
    for rec in (8, 40):
        assert b"zones_frames_kernelILi1024ELi4ELi%dELb1EE" % rec in blob and b"zones_frames_kernelILi1024ELi4ELi%dELb0EE" % rec in blob


def test_headers_compile_as_c_and_cpp_either_one_first(tmp_path):
    body = "int use(mtgpu_pipe *p, const uint64_t *k) { return mtgpu_pipe_set_keep(p, k) + mtgpu_pipe_has_keep(p); }\n"
    for first in ("mtgpu.h", "mtgpu_pipe_zones.h", "mtgpu_zones.h"):
        src = tmp_path / ("use_" + first.replace(".", "_") + ".c")
        src.write_text('#include "%s"\n#include "mtgpu_pipe_zones.h"\n%s' % (first, body))
        for comp, flag, lang in (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "c++")):
            subprocess.check_call([comp, flag, "-Wall", "-Werror", "-fsyntax-only", "-x", lang,
                                   "-I" + os.path.join(ROOT, "include"), str(src)])


def test_python_and_host_layer_expose_it():
    assert callable(m.ScanPipe.set_keep) and isinstance(m.ScanPipe.has_keep, property)
    for name in ("save_keep", "load_keep"):
        assert callable(getattr(zones, name)), name
    opts = {a.dest for a in zones.parser()._actions}
    assert {"mask", "mask_npy", "save_mask"} <= opts
    host = open(os.path.join(PKG, "csrc", "host", "mtgpu_host.hpp")).read()
    for text in ("void set_keep(std::vector<uint64_t> words)", "std::vector<uint64_t> keep;", "inline bool load_keep(",
                 "scanners[i]->set_keep(out.keep)"):
        assert text in host, text
    assert '"--keep"' in open(os.path.join(PKG, "csrc", "host", "mtgpu_scan_file.cpp")).read()


def test_plain_c_example_compiles():
    """examples/pipe_zones_example.c against the headers as they are (it runs in the GPU tier)."""
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "pipe_zones_example.c")])


def test_scan_file_refuses_a_bad_keep_option_before_any_device_call(tmp_path):
    exe = os.path.join(PKG, "mtgpu_scan_file")
    out = subprocess.run([exe, "x.mtmv", "--keep"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--keep takes the path" in out.stderr


# ------------------------------------------------------------------ .mtkeep

@pytest.fixture(scope="module")
def keep_loader(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keep_loader") / "keep_loader")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "keep_loader.cpp"),
                           "-o", exe, "-L" + PKG, "-lmtgpu", "-lpthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])

    def run(path, gw, gh):
        out = subprocess.run([exe, str(path), str(gw), str(gh)], capture_output=True, text=True, timeout=60)
        return out.returncode, out.stdout
    return run


def round_trip_masks():
    rng = np.random.RandomState(7)
    a = np.ones((68, 120), dtype=bool)                # the 1080p grid: a bit at x = 63 and one at x = 64 stand alone
    a[:] = False
    a[5, 63] = a[9, 64] = a[67, 119] = a[0, 0] = True
    b = rng.rand(9, 1) > 0.5                          # 1-wide
    b[0, 0], b[1, 0] = True, False
    c = rng.rand(5, 65) > 0.5                         # 65-wide: the second word holds one bit
    c[2, 64], c[3, 64] = True, False
    d = rng.rand(68, 120) > 0.3
    return [a, b, c, d]


@pytest.mark.parametrize("i", range(4), ids=["120-wide-seam", "1-wide", "65-wide", "120-wide-random"])
def test_mtkeep_round_trip_python_and_cpp(tmp_path, keep_loader, i):
    keep = round_trip_masks()[i]
    gh, gw = keep.shape
    path = tmp_path / "mask.mtkeep"
    zones.save_keep(str(path), keep)
    lines = path.read_text().split("\n")
    assert lines[0] == "mtkeep 1" and lines[1] == f"{gw} {gh}" and len(lines) == gh + 3 and lines[-1] == ""
    assert all(len(ln) == gw and set(ln) <= {"0", "1"} for ln in lines[2:-1])
    back = zones.load_keep(str(path))
    assert back.dtype == bool and np.array_equal(back, keep)
    assert np.array_equal(zones.load_keep(str(path), grid=(gw, gh)), keep)
    rc, out = keep_loader(path, gw, gh)
    assert rc == 0 and out.startswith("ok\n"), out
    words = np.array([[int(w, 16) for w in ln.split()] for ln in out.splitlines()[1:]], dtype=np.uint64)
    assert words.shape == (gh, (gw + 63) // 64) and np.array_equal(words, zones.pack_keep(keep))
    if i == 0:
        assert int(words[5, 0]) == 1 << 63 and int(words[9, 1]) == 1 and int(words[67, 1]) == 1 << (119 - 64)
    # a file a user edited on another system: CR LF line ends read the same
    path.write_text(path.read_text().replace("\n", "\r\n"))
    assert np.array_equal(zones.load_keep(str(path)), keep) and keep_loader(path, gw, gh)[1] == out


MALFORMED = [
    # (text, line named, words of the message) for a 3 x 2 grid
    ("mtkeeq 1\n3 2\n111\n111\n", 1, "mtkeep 1"),
    ("", 1, "mtkeep 1"),
    ("mtkeep 1\n", 2, "<grid_w> <grid_h>"),
    ("mtkeep 1\n3x2\n111\n111\n", 2, "<grid_w> <grid_h>"),
    ("mtkeep 1\n4 2\n1111\n1111\n", 2, "4x2 grid, this one is 3x2"),
    ("mtkeep 1\n3 3\n111\n111\n111\n", 2, "3x3 grid, this one is 3x2"),
    ("mtkeep 1\n3 2\n111\n", 4, "ends after 1 of 2 rows"),
    ("mtkeep 1\n3 2\n", 3, "ends after 0 of 2 rows"),
    ("mtkeep 1\n3 2\n111\n11\n", 4, "2 characters, want 3"),
    ("mtkeep 1\n3 2\n1111\n111\n", 3, "4 characters, want 3"),
    ("mtkeep 1\n3 2\n111\n1x1\n", 4, "character 2 is neither 0 nor 1"),
    ("mtkeep 1\n3 2\n1 1\n111\n", 3, "character 2 is neither 0 nor 1"),
    ("mtkeep 1\n3 2\n111\n112\n", 4, "character 3 is neither 0 nor 1"),
    ("mtkeep 1\n3 2\n111\n111\n111\n", 5, "behind the last of 2 rows"),
]


@pytest.mark.parametrize("i", range(len(MALFORMED)))
def test_malformed_mtkeep_is_refused_with_its_line(tmp_path, keep_loader, i):
    text, line, what = MALFORMED[i]
    path = tmp_path / "bad.mtkeep"
    path.write_text(text)
    with pytest.raises(ValueError) as e:
        zones.load_keep(str(path), grid=(3, 2))
    assert f"line {line}:" in str(e.value) and what in str(e.value), str(e.value)
    rc, out = keep_loader(path, 3, 2)
    assert rc == 3 and out.startswith("error ") and f"line {line}:" in out and what in out and out.endswith("words 0\n"), out


def test_load_keep_names_a_missing_file(tmp_path, keep_loader):
    rc, out = keep_loader(tmp_path / "none.mtkeep", 3, 2)
    assert rc == 3 and "cannot open" in out
    with pytest.raises(OSError):
        zones.load_keep(str(tmp_path / "none.mtkeep"))


def test_command_reads_and_writes_mtkeep_without_a_device(tmp_path, capsys):
    """--mask with a file for another grid ends with exit status 2 before a scanner is created; a malformed one with 1."""
    from mvtrim_amd import synth
    spec = synth.StreamSpec(width=320, height=240, block=16, sub=1, fps=30.0, gop=15, seed=2)
    frames = [synth.gen_frame(spec, i) for i in range(4)]
    src = str(tmp_path / "s.mtmv")
    m.mvfile.write_mtmv(src, 320, 240, 1, spec.tb_den, spec.fps, 4 / 30.0, [spec.pts_ticks(i) for i in range(4)], frames)
    other = str(tmp_path / "other.mtkeep")
    zones.save_keep(other, np.ones((4, 4), dtype=bool))
    with pytest.raises(SystemExit) as e:
        zones.main([src, "--mask", other])
    assert e.value.code == 2 and "4x4 grid, this one is 20x15" in capsys.readouterr().err
    bad = tmp_path / "bad.mtkeep"
    bad.write_text("mtkeep 1\n2 1\n1x\n")
    assert zones.main([src, "--mask", str(bad)]) == 1
    assert "line 3" in capsys.readouterr().err


# ------------------------------------------------------------------ the GPU tests' inputs against the oracle

def test_the_90_frame_input_has_every_kind_of_frame():
    p, frames, pts, keep_a, keep_b, want = pz.hd_case()
    assert p.vectors_needed == 1 and len(frames) == 90 == len(pts)
    (f0, c0), (fa, ca), (fb, cb) = want["none"], want["a"], want["b"]
    assert np.array_equal(f0, c0 >= p.clusters_needed) and np.array_equal(fa, ca >= p.clusters_needed)
    assert int(((f0 == 1) & (fa == 0)).sum()) >= 10                      # the mask turns the flag off
    assert int(((fa == 1) & (ca < c0)).sum()) >= 10                      # the flag stays, the count shrinks
    assert int(((ca == c0) & (c0 > 0)).sum()) >= 10                      # the zone is elsewhere: nothing changes
    none = [i for i, f in enumerate(frames) if f is None]
    assert none == [0, 30, 60] and not c0[none].any() and not ca[none].any()
    assert frames[pz.EMPTY_FRAME] is not None and len(frames[pz.EMPTY_FRAME]) == 0 and ca[pz.EMPTY_FRAME] == 0
    assert len(frames[pz.DENSE_FRAME]) == 4 * 8160 and max(len(f) for i, f in enumerate(frames) if f is not None and i != pz.DENSE_FRAME) == 8160
    assert len(set(ca.tolist())) >= 4
    # mask B is another recording's: it changes other frames than A does
    assert (ca != cb).any() and (cb != c0).any() and not np.array_equal(fa, fb)
    # and the numpy restatement of the AND rule gives the same counts as record removal
    mv, off, sd = pz.batch_arrays(list(frames))
    model, model_all = zi.model_batch(p, mv, off, sd, [0, 90], keep_a[None])
    assert np.array_equal(model, ca) and np.array_equal(model_all, c0)


def test_the_small_inputs_hold_their_hand_counts():
    p, one, two, keep = pz.stale_case()
    assert pz.expect(p, list(one), keep)[1].tolist() == [2] * 12 and pz.expect(p, list(one), keep)[0].all()
    assert pz.expect(p, list(two), None)[1].tolist() == [0, 3] * 6              # the motion is there ...
    assert not pz.expect(p, list(two), keep)[1].any()                            # ... and the zone removes all of it
    p, frames, cases = pz.seam_case()
    for keep, hand in cases:
        assert pz.expect(p, list(frames), keep)[1].tolist() == list(hand)
    p, frames, keep, hand = pz.vn0_case()
    mv, off, sd = pz.batch_arrays(list(frames))
    assert zi.model_batch(p, mv, off, sd, [0, 1], keep[None])[0].tolist() == list(hand)
    p, frames, keep, (fl, ce) = pz.uhd_case()
    plain = pz.expect(p, list(frames), None)[1]
    assert (ce < plain).sum() >= 6 and (ce > 0).sum() >= 6 and any(f is None for f in frames)
    p, frames, keep, hand = pz.tall_case()
    assert p.grid_h * ((p.grid_w + 63) // 64) > 1024                             # more keep words than lanes
    assert pz.expect(p, list(frames), keep)[1].tolist() == list(hand) and pz.expect(p, list(frames), None)[1].tolist() == [6, 2]
    # the grid without a masked form is the one mtgpu_zones_preview rejects
    with pytest.raises(m.MtgpuError) as e:
        m.zones_preview(m.ScanParams.from_config(3840, 2160, **pz.FINE_KW))
    assert e.value.code == _abi.MT_ERR_UNSUPPORTED and "960x540" in str(e.value)
