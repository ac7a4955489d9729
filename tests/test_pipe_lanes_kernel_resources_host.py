"""What the compiler reports for the pipe form of the plane scan, lanes_pipe_kernel in csrc/lanes_kernels.hip (CPU tier:
hipcc cross-compiles gfx950 without a GPU), by the method of tests/test_lanes_kernel_resources_host.py: the unit is
compiled with the library's own flags plus -Rpass-analysis=kernel-resource-usage and the remarks are parsed; no
instruction text is read.

The pipe form has four instantiations — 8- and 40-byte records, the plane's rows staged in LDS or read from memory.  Each
is held to what include/mtgpu_pipe_lanes.h counts on: no scratch, no spilled VGPR, no spilled SGPR (round 21 met one in
the direction scan's pipe form), occupancy 8."""
import pytest

from test_derived_kernel_resources_host import compile_unit
from test_scan_kernel_resources_host import makefile_flags

KERNEL = "lanes_pipe_kernel"


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled name of an instantiation: {remark field: int}}"""
    hipcc, flags = makefile_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    out = str(tmp_path_factory.mktemp("pipe_lanes_res") / "lanes_kernels.o")
    _, compiled = compile_unit(("lanes", hipcc, flags, out))
    return {n: r for n, r in compiled.items() if KERNEL in n}


def test_every_form_is_instantiated(resources):
    assert len(resources) == 4, sorted(resources)
    # <BLOCK, UNROLL, REC, STAGED>: both record sizes, both forms
    tails = sorted(n.split(KERNEL + "ILi1024ELi4E")[1][:9] for n in resources)
    assert tails == ["Li40ELb0E", "Li40ELb1E", "Li8ELb0EE", "Li8ELb1EE"], tails
    # the resident form's own test counts every symbol that contains its name: this one must not
    assert not any("lanes_frames_kernel" in n for n in resources)


def test_no_scratch_no_spill_eight_waves(resources):
    assert resources
    for n, r in sorted(resources.items()):
        print(n, r)
    for n, r in sorted(resources.items()):
        assert r["ScratchSize"] == 0, (n, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (n, r)
        assert r["Occupancy"] == 8, (n, r)
