"""What the compiler reports for the scan's seven derived kernel units — csrc/sweep_, activity_, zones_, blobs_, gmc_,
gmc_blobs_ and dir_kernels.hip (CPU tier: hipcc cross-compiles gfx950 without a GPU; the units compile side by side, in
a few seconds).  Their device passes are shared texts (record_stream.h, blob_label.h), so an edit to one
helper is an edit to every kernel that includes it: this test holds each `*_frames_kernel` instantiation to no scratch,
no spilled VGPR and the occupancy its family had, and counts the instantiations so that a dropped form is noticed.
Resource numbers only: each unit is compiled with the library's own flags plus -Rpass-analysis=kernel-resource-usage and
the remarks are parsed; no instruction text is read.

The floors are what the build of commit 7850179 — the parent of the commit that made the passes one text — reports,
taken before that commit's code was first compiled.  The kernels' comments plan on eight waves per SIMD; the activity map's form
without accumulators (ACC 0: the 4K form, one workgroup fills the CU's LDS and keeps its registers) is compiled for
four to eight and reports six, and that is its floor.

At 7850179 two forms missed the first assertion: activity_frames_kernel<1024, 4, 8, 16> and <1024, 4, 8, 32>, the
compact-record forms with accumulators, reported ScratchSize 20 and VGPRs Spill 4 (63 VGPRs under the 64 of eight waves
per SIMD).  Those two forms now make the zeros of their tile fill per frame (activity_kernels.hip says why) and report 0
and 0 like the rest."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_scan_kernel_resources_host import CSRC, makefile_flags

# unit -> (kernel, instantiations).  sweep: 2 record forms x 4 threshold counts; activity: 2 x 3 accumulator widths;
# zones, gmc, dir: 2 x {resident, pipe}; blobs, gmc_blobs: those four and the two boxed pipe forms.
UNITS = {
    "sweep": ("sweep_frames_kernel", 8),
    "activity": ("activity_frames_kernel", 6),
    "zones": ("zones_frames_kernel", 4),
    "blobs": ("blobs_frames_kernel", 6),
    "gmc": ("gmc_frames_kernel", 4),
    "gmc_blobs": ("gmc_blobs_frames_kernel", 6),
    "dir": ("dir_frames_kernel", 4),
}


def occupancy_floor(unit, name):
    """Waves per SIMD reported at 7850179 (see above): eight everywhere but the activity map's ACC 0 forms."""
    if unit == "activity" and re.search(r"activity_frames_kernelILi\d+ELi\d+ELi\d+ELi0EE", name):
        return 6
    return 8


def compile_unit(args):
    unit, hipcc, flags, out = args
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                          unit + "_kernels.hip", "-o", out],
                       cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stderr[-4000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        mo = re.search(r"remark:\s+Function Name: (\S+)", line)
        if mo:
            cur = res.setdefault(mo.group(1), {})
            continue
        mo = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass-analysis", line)
        if mo and cur is not None:
            cur[mo.group(1).strip()] = int(mo.group(2))
    return unit, res


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{unit: {mangled name of a *_frames_kernel instantiation: {remark field: int}}}"""
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    tmp = tmp_path_factory.mktemp("derived_res")
    jobs = [(u, hipcc, flags, str(tmp / (u + "_kernels.o"))) for u in UNITS]
    with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
        compiled = dict(pool.map(compile_unit, jobs))
    return {u: {n: r for n, r in compiled[u].items() if UNITS[u][0] in n} for u in UNITS}


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_every_form_is_instantiated(resources, unit):
    assert len(resources[unit]) == UNITS[unit][1], sorted(resources[unit])


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_no_frames_kernel_uses_scratch(resources, unit):
    assert resources[unit]
    for n, r in sorted(resources[unit].items()):
        print(n, r)
    for n, r in sorted(resources[unit].items()):
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (n, r)


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_frames_kernels_keep_their_occupancy(resources, unit):
    assert resources[unit]
    for n, r in sorted(resources[unit].items()):
        print(n, r)
        assert r["Occupancy"] >= occupancy_floor(unit, n), (n, r)
