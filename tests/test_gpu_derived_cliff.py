"""GPU tier (`-m gpu`): the sweep, the activity map, the masked scan, the compensated scan, the direction scan and the
plane scan (with the flow map) on the last grids their LDS layouts hold — two, three, 65 and 193 columns at the largest
height, one and three rows at the largest width, for the activity map the last and the first grid of every plan
outcome, and for the plane scan the last grid of its staged form and the first one behind it — through the C ABI's
device entry points on both record layouts.

The shapes, the batches and the values derived by hand come from tests/derived_cliff_inputs.py, which finds the shapes
with the previews at 163 840 bytes of LDS; tests/test_derived_cliff_host.py proves without a GPU that they sit on the
limit and that two independent sources agree on every expected value.  Here every comparison is exact, outputs are
pre-filled with junk, and the grid one row or column past each shape must be refused with every output byte untouched.
Every test first asserts that the context's LDS limit is the one the shapes were derived for."""
import re

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_cliff_inputs as dci
from activity_model import model_maps
from scan_checks import assert_counts_equal, to_device
from test_gpu_activity import assert_maps_equal, device_maps, junk_maps
from test_gpu_activity import JUNK as MAP_JUNK
from test_gpu_sweep import JUNK as SWEEP_JUNK
from test_gpu_sweep import device_sweep, junk_out
from test_gpu_zones import JUNK, JUNK_FLAG, keep_tensor, soff_tensor, zones_both_layouts

pytestmark = pytest.mark.gpu

_limit = []


def assert_lds_limit(gpu_scanner_factory):
    """The context's own limit, read from the message of a call it refuses: on another device the shapes below are not
    the last ones, and the tests must fail here instead of running off the limit."""
    if not _limit:
        big = gpu_scanner_factory(m.ScanParams.from_config(3840, 2160, block_size=4, block_shift=2))
        with pytest.raises(m.MtgpuError) as ei:
            big.scan_zones(m.FrameBatch(np.zeros(3, dtype=m.MV_DTYPE), np.array([0, 3], dtype=np.uint64)), [0, 1],
                           np.zeros((1, 540, 15), dtype=np.uint64))
        assert ei.value.code == _abi.MT_ERR_UNSUPPORTED
        found = re.search(r"fit (\d+) bytes of LDS", str(ei.value))
        assert found is not None, f"the refusal no longer states the context's LDS limit: {ei.value}"
        _limit.append(int(found.group(1)))
    assert _limit[0] == dci.MI355X_LDS, f"LDS per workgroup is {_limit[0]}: the limit shapes were derived for {dci.MI355X_LDS}"


def refused(call):
    import torch
    with pytest.raises(m.MtgpuError) as ei:
        call()
    torch.cuda.synchronize()
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED, ei.value


def untouched(t, junk):
    return int((t != junk).sum()) == 0


# ------------------------------------------------------------------ the masked scan

@pytest.mark.parametrize("name", list(dci.shapes("zones")))
def test_zones_at_the_lds_limit(gpu_scanner_factory, name):
    """Three streams — all ones, 30 % cleared at random, one cell of every seam pair cleared — flags, centres and
    centres_all against the oracle on filtered records (== the numpy AND rule, on the CPU) and the planted frames
    against their hand values.  Two, three and 65 columns: the keep words take a second trip of the staging loop."""
    import torch
    assert_lds_limit(gpu_scanner_factory)
    p, mv, off, sd, soff, keeps, hand = dci.zones_case(name)
    (want_f, want_c, want_all), _ = dci.zones_expected(p, mv, off, sd, soff, keeps)
    s = gpu_scanner_factory(p)
    for label, fl, ce, ca in zones_both_layouts(s, mv, off, sd, soff, keeps, name):
        assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
        assert_counts_equal(ca, want_all, label + " centres_all")
        for f, (hc, hca) in hand.items():
            assert (int(ce[f]), int(ca[f])) == (hc, hca), (label, "planted frame", f)
    gw, gh, kind = dci.shapes("zones")[name]
    mw, mh = dci.one_more(gw, gh, kind)
    more = gpu_scanner_factory(dci.grid_params(mw, mh, **dci.CTX_KW))
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    F = len(sd)
    fl = torch.full((F,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce, ca = (torch.full((F,), JUNK, dtype=torch.int32, device="cuda") for _ in range(2))
    d_keep = keep_tensor(np.ones((3, mh, mw), dtype=bool))
    refused(lambda: more.scan_zones_device(d_rec, d_off, d_sd, soff_tensor(soff), d_keep, compact=True, flags=fl, centres=ce,
                                           centres_all=ca))
    assert untouched(fl, JUNK_FLAG) and untouched(ce, JUNK) and untouched(ca, JUNK)


# ------------------------------------------------------------------ the activity map

@pytest.mark.parametrize("name", list(dci.shapes("activity")))
def test_activity_at_the_lds_limit(gpu_scanner_factory, name):
    """Two streams split mid-batch, min_centres 0 and 1, run_frames 0 and one that puts the stream boundary inside a run,
    against the numpy model (== the oracle's identities, on the CPU); then the planted frames alone against per-cell hand
    values.  The "plan" shapes are the last and the first grid of each outcome of activity_plan."""
    assert_lds_limit(gpu_scanner_factory)
    p, mv, off, sd, soff, _ = dci.activity_case(name)
    gw, gh, kind = dci.shapes("activity")[name]
    pv = m.activity_preview(p)
    s = gpu_scanner_factory(p)
    wants = {mc: model_maps(p, mv, off, sd, soff, mc)[:3] for mc in (0, 1)}
    pmv, poff, psd, psoff, ha, hc, hf = dci.activity_planted_case(name)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for mc in (0, 1):
            for run in (0, dci.ACT_RUN):
                got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(soff), compact, min_centres=mc, run_frames=run)
                assert_maps_equal(got, wants[mc], f"{name} {pv} compact {compact} min_centres {mc} run_frames {run}")
        d_rec, d_off, d_sd = to_device(pmv, poff, psd, compact)
        got = device_maps(s, d_rec, d_off, d_sd, soff_tensor(psoff), compact)
        assert_maps_equal(got, (ha, hc, hf), f"{name} planted frames by hand, compact {compact}")
    if kind == "plan":
        return
    more = gpu_scanner_factory(dci.grid_params(*dci.one_more(gw, gh, kind), **dci.CTX_KW))
    outs = junk_maps(more, 2)
    refused(lambda: more.activity_map_device(d_rec, d_off, d_sd, soff_tensor([0, 2, 4]), compact=True, out=outs))
    assert all(untouched(t, MAP_JUNK) for t in outs.values())


# ------------------------------------------------------------------ the sweep

@pytest.mark.parametrize("kernel,name", [(k, n) for k in ("sweep1", "sweep8") for n in dci.shapes(k)])
def test_sweep_at_the_lds_limit(gpu_scanner_factory, kernel, name):
    """1 x 1: the tile and a mask buffer fill the LDS, one call per setting (levels 0 and 255 among them).  8 x 8: eight
    passes of one tile next to a mask buffer of three rows or little more, thresholds and levels in the caller's order
    with duplicates.  Against the oracle per setting (== the numpy rule, on the CPU) and the planted frames' hand values."""
    assert_lds_limit(gpu_scanner_factory)
    gw, gh, kind = dci.shapes(kernel)[name]
    mv, off, sd, _ = dci.batch(gw, gh)
    s = gpu_scanner_factory(dci.grid_params(gw, gh))
    more = gpu_scanner_factory(dci.grid_params(*dci.one_more(gw, gh, kind)))
    print(kernel, name, "passes, chunk_rows, R", dci.sweep_path(kernel, name))
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(mv, off, sd, compact)
        for thr, vec in dci.sweep_calls(kernel):
            want = dci.sweep_expected(kernel, name, thr, vec)
            got = device_sweep(s, d_rec, d_off, d_sd, thr, vec, compact)
            assert_counts_equal(got.reshape(-1), want.reshape(-1), f"{kernel} {name} {thr} x {vec} compact {compact}")
            for f, h in dci.sweep_hand(kernel, name, thr, vec).items():
                assert np.array_equal(got[:, :, f], h), (kernel, name, "planted frame", f, thr, vec)
    thr, vec = dci.sweep_calls(kernel)[0]
    out = junk_out(len(thr), len(vec), len(sd))
    refused(lambda: more.sweep_centres_device(d_rec, d_off, d_sd, thr, vec, compact=True, out=out))
    assert untouched(out, SWEEP_JUNK)


# ------------------------------------------------------------------ the compensated scan

@pytest.mark.parametrize("name", list(dci.shapes("gmc")))
def test_gmc_at_the_lds_limit(gpu_scanner_factory, name):
    """The histograms and the result words are the last things in the LDS, behind the tile and the mask plane: on the
    last grid that fits, the shape's batch with max_shift 0 and with the defaults — centres, flags and info against the
    numpy model, centres against the oracle on src-shifted records (consequence C; == the model, on the CPU) — then two
    planted frames under a pan of (7, -3) against their hand values, then the grid one row or column further."""
    import torch
    from test_gpu_gmc import assert_info_equal, gmc_both_layouts
    assert_lds_limit(gpu_scanner_factory)
    gw, gh, kind = dci.shapes("gmc")[name]
    mv, off, sd, _ = dci.batch(gw, gh)
    s = gpu_scanner_factory(dci.grid_params(gw, gh, **dci.CTX_KW))
    for ms, q8 in dci.GMC_SETTINGS:
        want_f, want_c, want_i = dci.gmc_expected(gw, gh, ms, q8)
        fits, oracle_c = dci.gmc_oracle_c(gw, gh, want_i)
        for label, fl, ce, info in gmc_both_layouts(s, mv, off, sd, ms, q8, f"{name} max_shift {ms}"):
            assert_counts_equal(ce, want_c, label, got_f=fl, want_f=want_f)
            assert_info_equal(info, want_i, label)
            assert_counts_equal(ce[fits], oracle_c[fits], label + " (C)")
    pp, pmv, poff, psd, hand_c, hand_i = dci.gmc_pan_case(name)
    ps = gpu_scanner_factory(pp)
    for label, fl, ce, info in gmc_both_layouts(ps, pmv, poff, psd, dci.GMC_PAN_MAX_SHIFT, 128, name + " planted pan"):
        assert_counts_equal(ce, hand_c, label, got_f=fl, want_f=(hand_c >= 2).astype(np.uint8))
        assert_info_equal(info, hand_i, label)
    more = gpu_scanner_factory(dci.grid_params(*dci.one_more(gw, gh, kind), **dci.CTX_KW))
    d_rec, d_off, d_sd = to_device(mv, off, sd, True)
    F = len(sd)
    fl = torch.full((F,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce = torch.full((F,), JUNK, dtype=torch.int32, device="cuda")
    inf = torch.full((F, 5), JUNK, dtype=torch.int32, device="cuda")
    refused(lambda: more.scan_gmc_device(d_rec, d_off, d_sd, 16, 128, compact=True, flags=fl, centres=ce, info=inf))
    assert untouched(fl, JUNK_FLAG) and untouched(ce, JUNK) and untouched(inf, JUNK)


# ------------------------------------------------------------------ the direction scan

@pytest.mark.parametrize("name", list(dci.shapes("dir")))
def test_dir_at_the_lds_limit(gpu_scanner_factory, name):
    """The rose words are the last things in the LDS, behind the tile, the mask plane and the totals: on the last grid
    that fits, the directed batch under nothing, the even sectors, the odd sectors and everything, then under one byte
    per stream — flags, centres and roses against the numpy model (== the oracle on filtered records, on the CPU), the
    planted frames against their hand values — then the grid one row or column further."""
    from test_gpu_dir import assert_equals_model, device_dir, junk_outputs
    assert_lds_limit(gpu_scanner_factory)
    gw, gh, kind = dci.shapes("dir")[name]
    c = dci.dir_case(name)
    s = gpu_scanner_factory(c["params"])
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        for allow in dci.DIR_CHAIN + (None,):
            kw = dict(soff=c["soff"], allows=c["allows"]) if allow is None else dict(allow=allow)
            label = f"{name} allow {'per stream' if allow is None else hex(allow)} compact {compact}"
            got = device_dir(s, d_rec, d_off, d_sd, compact, **kw)
            assert_equals_model(got, dci.dir_expected(name, allow), label)
            for f, (hc, hr) in dci.dir_hand(c, allow).items():
                assert int(got[1][f]) == hc and got[2][f].tolist() == hr.tolist(), (label, "planted frame", f)
    more = gpu_scanner_factory(dci.grid_params(*dci.one_more(gw, gh, kind), **dci.CTX_KW))
    out = junk_outputs(len(c["sd"]))
    refused(lambda: more.scan_dir_device(d_rec, d_off, d_sd, allow=0xFF, compact=True, out=out))
    assert untouched(out["flags"], JUNK_FLAG) and untouched(out["centres"], JUNK) and untouched(out["rose"], JUNK)


# ------------------------------------------------------------------ the plane scan and the flow map

def planes_at(planes, shift):
    """The planes in device memory `shift` bytes behind an allocation's start, as a contiguous uint8 tensor (what
    test_gpu_derived_edges.shifted does for records, whose shifts are 4 modulo 8; a plane takes any byte)."""
    import torch
    flat = np.ascontiguousarray(planes, dtype=np.uint8).reshape(-1)
    room = torch.zeros(flat.size + 8, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    view = room[shift:shift + flat.size]
    view.copy_(torch.from_numpy(flat.copy()))
    assert view.data_ptr() % 4 == shift % 4 and view.is_contiguous()
    return view


def device_lanes_at(s, d_rec, d_off, d_sd, compact, planes, soff, shift):
    """Through mtgpu_scan_lanes_device with the plane tensor at `shift`, into junk-filled outputs."""
    import torch
    from test_gpu_dir import junk_outputs
    n = d_off.numel() - 1
    out = junk_outputs(n)
    d_planes = planes_at(planes, shift)
    torch.cuda.synchronize()
    s.scan_lanes_device(d_rec, d_off, d_sd, d_planes, d_stream_off=soff_tensor(soff), compact=compact, out=out)
    torch.cuda.synchronize()
    return out["flags"].cpu().numpy(), out["centres"].cpu().numpy().view(np.uint32), out["rose"].cpu().numpy().view(np.uint32).reshape(n, 8)


def assert_lanes_case(s, c, name, rotation, want, d_rec, d_off, d_sd, compact, shift):
    from test_gpu_dir import assert_equals_model
    label = f"{name} planes {rotation} at byte {shift} compact {compact}"
    got = device_lanes_at(s, d_rec, d_off, d_sd, compact, dci.lanes_stack(c, rotation), c["soff"], shift)
    assert_equals_model(got, want, label)
    for f, (hc, hr) in dci.lanes_hand(c, rotation).items():
        assert (hc is None or int(got[1][f]) == hc) and got[2][f].tolist() == hr.tolist(), (label, "planted frame", f)


@pytest.mark.parametrize("name", list(dci.shapes("lanes")))
def test_lanes_at_the_lds_limit(gpu_scanner_factory, name):
    """The staged plane rows are the last bytes of the LDS: on the last staged grid, the first unstaged one and the last
    one that fits at all, three streams under P_all, P_own and P_half in every rotation (stream s reads plane s, whose
    rows start (s gh) gw bytes into the tensor; the tensor starts 1, 2 and 3 bytes behind an allocation) — flags,
    centres and roses against the numpy model (== the oracle on filtered records, on the CPU), the planted frames against
    their hand values: the corner pairs hold the first and the last bytes of the copy.  Then the flow map of the same
    batch per stream and per frame, the planted frames' maps by hand; then, on the last grid, one row or column further."""
    from test_gpu_dir import junk_outputs
    from test_gpu_lanes import assert_flow_equal, device_flow
    import torch
    assert_lds_limit(gpu_scanner_factory)
    gw, gh, kind = dci.shapes("lanes")[name]
    c = dci.lanes_case(name)
    assert m.lanes_preview(c["params"])["staged"] == (1 if "-staged-" in name else 0)
    s = gpu_scanner_factory(c["params"])
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        for i, rot in enumerate(dci.LANES_ROTATIONS):
            assert_lanes_case(s, c, name, rot, dci.lanes_expected(name, rot), d_rec, d_off, d_sd, compact, i + 1)
        for soff in (dci.ZONE_SOFF, dci.FLOW_EACH):
            got = device_flow(s, d_rec, d_off, d_sd, compact, list(soff))
            assert_flow_equal(got, dci.flow_expected(name, soff), f"{name} flow map, {len(soff) - 1} streams, compact {compact}")
        for f, n in enumerate(dci.ORDER):                            # got: one stream per frame
            if n in c["planted"]:
                assert np.array_equal(got[f], dci.hand_flow(c["planted"][n], gw, gh)), (name, "planted frame's flow map", f)
    if kind == "plan":
        return
    mw, mh = dci.one_more(gw, gh, kind)
    more = gpu_scanner_factory(dci.grid_params(mw, mh, **dci.CTX_KW))
    out = junk_outputs(len(c["sd"]))
    d_planes = planes_at(np.full((3, mh, mw), 0xFF, dtype=np.uint8), 0)
    refused(lambda: more.scan_lanes_device(d_rec, d_off, d_sd, d_planes, d_stream_off=soff_tensor(c["soff"]), compact=True, out=out))
    assert untouched(out["flags"], JUNK_FLAG) and untouched(out["centres"], JUNK) and untouched(out["rose"], JUNK)
    flow = torch.full((3, 8, mh, mw), JUNK, dtype=torch.int32, device="cuda")
    refused(lambda: more.flow_map_device(d_rec, d_off, d_sd, soff_tensor(c["soff"]), compact=True, out=flow))
    assert untouched(flow, JUNK)


@pytest.mark.parametrize("name,margin", dci.phase_runs(), ids=[f"{n}-margin{mg}" for n, mg in dci.phase_runs()])
def test_lanes_plane_base_phases(gpu_scanner_factory, name, margin):
    """The three-stream call with the plane tensor 0, 1, 2 and 3 bytes behind an allocation's start: over the runs the
    staged copy meets every source phase with 0, 1, 2 and 3 tail bytes (tests/test_derived_cliff_host.py).  The run with a
    margin copies rows y_lo .. y_hi - 1 only, and its planted pairs sit on those rows."""
    assert_lds_limit(gpu_scanner_factory)
    c = dci.lanes_case(name, margin)
    s = gpu_scanner_factory(c["params"])
    want = dci.lanes_expected(name, dci.PHASE_ROTATION, margin)
    for shift in dci.PHASE_SHIFTS:
        compact = bool(shift % 2)
        d_rec, d_off, d_sd = to_device(c["mv"], c["off"], c["sd"], compact)
        assert_lanes_case(s, c, f"{name} margin {margin}", dci.PHASE_ROTATION, want, d_rec, d_off, d_sd, compact, shift)
