"""What the compiler reports for csrc/lanes_kernels.hip (CPU tier: hipcc cross-compiles gfx950 without a GPU), by the method
of tests/test_derived_kernel_resources_host.py: the unit is compiled with the library's own flags plus
-Rpass-analysis=kernel-resource-usage and the remarks are parsed; no instruction text is read.

The plane scan has four forms — 8- and 40-byte records, the plane's rows staged in LDS or read from memory — and the flow
map two.  Each is held to the floor every sibling compiled for eight waves per SIMD is held to: no scratch, no spilled
VGPR, occupancy 8 (two workgroups of 1024 lanes per CU, which mtgpu_lanes.h's size table counts on for 1080p)."""
import pytest

from test_derived_kernel_resources_host import compile_unit
from test_scan_kernel_resources_host import makefile_flags

KERNELS = {"lanes_frames_kernel": 4, "flow_frames_kernel": 2}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{kernel: {mangled name of an instantiation: {remark field: int}}}"""
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    out = str(tmp_path_factory.mktemp("lanes_res") / "lanes_kernels.o")
    _, compiled = compile_unit(("lanes", hipcc, flags, out))
    return {k: {n: r for n, r in compiled.items() if k in n} for k in KERNELS}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_form_is_instantiated(resources, kernel):
    assert len(resources[kernel]) == KERNELS[kernel], sorted(resources[kernel])
    if kernel == "lanes_frames_kernel":       # <BLOCK, UNROLL, REC, STAGED>: both record sizes, both forms
        tails = sorted(n.split("lanes_frames_kernelILi1024ELi4E")[1][:9] for n in resources[kernel])
        assert tails == ["Li40ELb0E", "Li40ELb1E", "Li8ELb0EE", "Li8ELb1EE"], tails


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_no_scratch_no_spill_eight_waves(resources, kernel):
    assert resources[kernel]
    for n, r in sorted(resources[kernel].items()):
        print(n, r)
    for n, r in sorted(resources[kernel].items()):
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (n, r)
        assert r["Occupancy"] == 8, (n, r)
