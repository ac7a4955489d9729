"""Soak of the derived kernels: randomised parity of the sweep, the activity map, the masked scan, the compensated scan,
the blob scan, the compensated blob scan, the direction scan, the plane scan and the flow map for MTGPU_SOAK_SECONDS
(default 4 s; set it to minutes to hunt rare faults).
Every iteration draws a grid, a parameter set, a ragged batch with runs and blobs, streams with empty ones, keep masks,
sweep settings, a pan per frame with max_shift and min_share_q8, a minimum blob size, whether the blob scans are masked,
an allow byte, bytes and planes per stream with the forms of their calls, a record layout and — every third time — a record base inside a larger buffer
(tests/derived_soak.py, which also computes the expected values from the oracle and the numpy models and rebuilds any
iteration on the CPU: derived_soak.replay(seed, it)).  Every comparison is exact; a kernel whose preview says
unsupported must answer MT_ERR_UNSUPPORTED and touch nothing."""
import os
import time

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_soak as dsoak
import test_gpu_gmc_blobs as gb
from scan_checks import assert_counts_equal
from test_gpu_activity import assert_maps_equal, junk_maps
from test_gpu_derived_cliff import assert_lds_limit
from test_gpu_derived_edges import shifted
from test_gpu_dir import assert_equals_model
from test_gpu_dir import junk_outputs as dir_junk_outputs
from test_gpu_gmc import assert_info_equal
from test_gpu_lanes import assert_flow_equal, odd_planes
from test_gpu_zones import keep_tensor, soff_tensor

pytestmark = pytest.mark.gpu

JUNK, JUNK_FLAG = -7, 9


def records_on_device(d, mv=None):
    """The records (mv: another copy of them, record for record) in the draw's layout; on a window iteration inside a
    larger buffer: 40-byte records shifted by 4, 12 or 20 bytes, compact ones with the first record on the drawn 8-byte
    residue of a 128-byte line."""
    import torch
    mv, compact = d["mv"] if mv is None else mv, d["compact"]
    raw = (m.pack_records(mv) if compact else np.ascontiguousarray(mv, dtype=m.MV_DTYPE)).view(np.uint8).reshape(-1)
    host = torch.from_numpy(raw.copy())
    if d["window"] is None or raw.size == 0:
        return host.cuda() if raw.size else torch.zeros(0, dtype=torch.uint8, device="cuda")
    if not compact:
        return shifted(host, d["window"][0])
    buf = torch.zeros(raw.size + 256, dtype=torch.uint8, device="cuda")
    at = (d["window"][1] - buf.data_ptr()) % 128
    view = buf[at:at + raw.size]
    view.copy_(host)
    assert view.data_ptr() % 128 == d["window"][1]
    return view


def expect_unsupported(call, outs, junks, what):
    import torch
    with pytest.raises(m.MtgpuError) as ei:
        call()
    torch.cuda.synchronize()
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED, (what, ei.value)
    for t, j in zip(outs, junks):
        assert int((t != j).sum()) == 0, (what, "a refused call wrote to an output")


def check_draw(s, d, where):
    import torch
    F, compact = len(d["sd"]), d["compact"]
    d_rec = records_on_device(d)
    d_off = torch.from_numpy(d["off"].astype(np.int64)).cuda()
    d_sd = torch.from_numpy(d["sd"]).cuda()
    gh, gw = d["params"].grid_h, d["params"].grid_w
    # the sweep
    out = torch.full((len(d["thr"]), len(d["vec"]), F), JUNK, dtype=torch.int32, device="cuda")
    call = lambda: s.sweep_centres_device(d_rec, d_off, d_sd, d["thr"], d["vec"], compact=compact, out=out)   # noqa: E731
    if d["support"]["sweep"]:
        call()
        torch.cuda.synchronize()
        want = dsoak.expected(d, "sweep")["centres"]
        assert_counts_equal(out.cpu().numpy().view(np.uint32).reshape(-1), want.reshape(-1), f"sweep {d['thr']} x {d['vec']}, {where}")
    else:
        expect_unsupported(call, [out], [JUNK], "sweep, " + where)
    # the activity map
    outs = junk_maps(s, len(d["soff"]) - 1)
    call = lambda: s.activity_map_device(d_rec, d_off, d_sd, soff_tensor(d["soff"]), min_centres=d["min_centres"],   # noqa: E731
                                         run_frames=d["run_frames"], compact=compact, out=outs)
    if d["support"]["activity"]:
        call()
        torch.cuda.synchronize()
        got = tuple(outs[n].cpu().numpy().view(np.uint32) for n in ("active", "centre", "frames"))
        assert_maps_equal(got, dsoak.expected(d, "activity")["maps"],
                          f"activity min_centres {d['min_centres']} run_frames {d['run_frames']} streams {d['soff'].tolist()}, {where}")
    else:
        expect_unsupported(call, list(outs.values()), [JUNK] * 3, "activity, " + where)
    # the masked scan
    fl = torch.full((F,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce, ca = (torch.full((F,), JUNK, dtype=torch.int32, device="cuda") for _ in range(2))
    S = len(d["zsoff"]) - 1
    keeps = d["keeps"] if d["keeps"] is not None else np.ones((S, gh, gw), dtype=bool)
    d_keep = keep_tensor(keeps)
    call = lambda: s.scan_zones_device(d_rec, d_off, d_sd, soff_tensor(d["zsoff"]), d_keep, compact=compact, flags=fl,   # noqa: E731
                                       centres=ce, centres_all=ca)
    if d["support"]["zones"]:
        call()
        torch.cuda.synchronize()
        e = dsoak.expected(d, "zones")
        what = f"zones streams {d['zsoff'].tolist()} densities {d['keep_density']}, {where}"
        assert_counts_equal(ce.cpu().numpy().view(np.uint32), e["centres"], what, got_f=fl.cpu().numpy(), want_f=e["flags"])
        assert_counts_equal(ca.cpu().numpy().view(np.uint32), e["centres_all"], what + " centres_all")
    else:
        expect_unsupported(call, [fl, ce, ca], [JUNK_FLAG, JUNK, JUNK], "zones, " + where)
    # the compensated scan, on its own copy of the records at the same base
    g_rec = records_on_device(d, d["gmc_mv"])
    fl = torch.full((F,), JUNK_FLAG, dtype=torch.uint8, device="cuda")
    ce = torch.full((F,), JUNK, dtype=torch.int32, device="cuda")
    inf = torch.full((F, 5), JUNK, dtype=torch.int32, device="cuda")
    call = lambda: s.scan_gmc_device(g_rec, d_off, d_sd, d["gmc_max_shift"], d["gmc_share_q8"], compact=compact, flags=fl,   # noqa: E731
                                     centres=ce, info=inf)
    if d["support"]["gmc"]:
        call()
        torch.cuda.synchronize()
        e = dsoak.expected(d, "gmc")
        what = f"gmc max_shift {d['gmc_max_shift']} min_share_q8 {d['gmc_share_q8']} follow {d['gmc_follow']}, {where}"
        assert_counts_equal(ce.cpu().numpy().view(np.uint32), e["centres"], what, got_f=fl.cpu().numpy(), want_f=e["flags"])
        assert_info_equal(inf.cpu().numpy().reshape(-1).view(_abi.GMC_INFO_DTYPE), e["info"], what)
        reached = {"gmc": e}
    else:
        expect_unsupported(call, [fl, ce, inf], [JUNK_FLAG, JUNK, JUNK], "gmc, " + where)
        reached = {"gmc": None}
    # the blob scan on the draw's records and the compensated blob scan on the compensated scan's copy: min_blob_cells and
    # the mask decision of the draw, the draw's layout and base, all outputs requested
    soff, keeps = dsoak.blob_masks(d)
    b_soff, b_keep = (soff_tensor(soff), keep_tensor(keeps)) if keeps is not None else (None, None)
    mb = d["min_blob_cells"]
    masks = f"min_blob_cells {mb} masked {keeps is not None}" + (f" streams {soff.tolist()} densities {d['keep_density']}" if keeps is not None else "")
    for kernel, rec in (("blobs", d_rec), ("gmc_blobs", g_rec)):
        out = gb.junk_outputs(F, gb.OUTPUTS if kernel == "gmc_blobs" else gb.BLOB_OUTPUTS)
        if kernel == "blobs":
            call = lambda: s.scan_blobs_device(rec, d_off, d_sd, mb, b_soff, b_keep, compact=compact, out=out)   # noqa: E731
        else:
            call = lambda: s.scan_gmc_blobs_device(rec, d_off, d_sd, d["gmc_max_shift"], d["gmc_share_q8"], mb, b_soff, b_keep,   # noqa: E731
                                                   compact=compact, out=out)
        if d["support"][kernel]:
            call()
            torch.cuda.synchronize()
            e = dsoak.expected(d, kernel)
            what = f"{kernel} {masks}" + (f" max_shift {d['gmc_max_shift']} min_share_q8 {d['gmc_share_q8']}" if kernel == "gmc_blobs" else "") + ", " + where
            got = gb.to_host(out)
            gb.assert_blobs(got, e, what)
            assert got["flags"].tolist() == e["flags"].tolist(), (what, "flags", got["flags"].tolist(), e["flags"].tolist())
            if kernel == "gmc_blobs":
                gb.assert_info(got, e["info"], what)
            reached[kernel] = e
        else:
            expect_unsupported(call, list(out.values()), [{"flags": JUNK_FLAG, "box": gb.JUNK_BOX}.get(k, JUNK) for k in out], kernel + ", " + where)
            reached[kernel] = None
    # the direction scan and the plane scan on the draw's records, layout and base: the drawn byte(s) or plane(s) in the
    # drawn form, then allow 0xFF and a plane of 0xFF, which must give the oracle's plain counts
    def rose_outputs(out):
        return out["flags"].cpu().numpy(), out["centres"].cpu().numpy().view(np.uint32), out["rose"].cpu().numpy().view(np.uint32).reshape(F, 8)

    junks = [JUNK_FLAG, JUNK, JUNK]
    z_soff = soff_tensor(d["zsoff"])
    out = dir_junk_outputs(F)
    if d["dir_per_stream"]:
        d_allow = torch.from_numpy(np.concatenate([d["allows"], np.zeros(1, dtype=np.uint8)])).cuda()
        call = lambda: s.scan_dir_device(d_rec, d_off, d_sd, d_stream_off=z_soff, d_allow=d_allow, compact=compact, out=out)   # noqa: E731
        what = f"dir streams {d['zsoff'].tolist()} bytes {d['allows'].tolist()}, {where}"
    else:
        call = lambda: s.scan_dir_device(d_rec, d_off, d_sd, allow=d["allow"], compact=compact, out=out)   # noqa: E731
        what = f"dir byte {d['allow']:#x}, {where}"
    if d["support"]["dir"]:
        call()
        torch.cuda.synchronize()
        e = dsoak.expected(d, "dir")
        assert_equals_model(rose_outputs(out), (e["flags"], e["centres"], e["rose"]), what)
        out = dir_junk_outputs(F)
        s.scan_dir_device(d_rec, d_off, d_sd, allow=0xFF, compact=compact, out=out)
        torch.cuda.synchronize()
        fl, ce, _ = rose_outputs(out)
        assert_counts_equal(ce, e["plain"][1], "dir byte 0xff against the oracle, " + where, got_f=fl, want_f=e["plain"][0])
        reached["dir"] = e
    else:
        expect_unsupported(call, list(out.values()), junks, "dir, " + where)
        reached["dir"] = None
    out = dir_junk_outputs(F)
    S = len(d["zsoff"]) - 1
    planes = d["planes"] if d["planes"] is not None else np.full((S, gh, gw), 0xFF, dtype=np.uint8)
    if d["lanes_one_plane"]:
        d_planes = odd_planes(planes[0])
        call = lambda: s.scan_lanes_device(d_rec, d_off, d_sd, d_planes, compact=compact, out=out)   # noqa: E731
        what = f"lanes one plane ({(d['plane_kinds'] or ['-'])[0]}), {where}"
    else:
        d_planes = odd_planes(planes)
        call = lambda: s.scan_lanes_device(d_rec, d_off, d_sd, d_planes, d_stream_off=z_soff, compact=compact, out=out)   # noqa: E731
        what = f"lanes streams {d['zsoff'].tolist()} planes {d['plane_kinds']}, {where}"
    if d["support"]["lanes"]:
        call()
        torch.cuda.synchronize()
        e = dsoak.expected(d, "lanes")
        assert_equals_model(rose_outputs(out), (e["flags"], e["centres"], e["rose"]), what)
        out = dir_junk_outputs(F)
        s.scan_lanes_device(d_rec, d_off, d_sd, odd_planes(np.full((gh, gw), 0xFF, dtype=np.uint8)), compact=compact, out=out)
        torch.cuda.synchronize()
        fl, ce, _ = rose_outputs(out)
        assert_counts_equal(ce, e["plain"][1], "lanes plane 0xff against the oracle, " + where, got_f=fl, want_f=e["plain"][0])
        reached["lanes"] = dict(e, unstaged=int(d["lanes_staged"] == 0))
    else:
        expect_unsupported(call, list(out.values()), junks, "lanes, " + where)
        reached["lanes"] = None
    # the flow map over the activity map's streams
    flow = torch.full((len(d["soff"]) - 1, 8, gh, gw), JUNK, dtype=torch.int32, device="cuda")
    call = lambda: s.flow_map_device(d_rec, d_off, d_sd, soff_tensor(d["soff"]), compact=compact, out=flow)   # noqa: E731
    if d["support"]["flow"]:
        call()
        torch.cuda.synchronize()
        assert_flow_equal(flow.cpu().numpy().view(np.uint32), dsoak.expected(d, "flow")["flow"], f"flow map streams {d['soff'].tolist()}, {where}")
    else:
        expect_unsupported(call, [flow], [JUNK], "flow, " + where)
    return reached


def test_soak_derived_kernels(gpu_scanner_factory):
    assert_lds_limit(gpu_scanner_factory)
    budget = float(os.environ.get("MTGPU_SOAK_SECONDS", "4"))
    seed = int(os.environ.get("MTGPU_SOAK_SEED", str(dsoak.DEFAULT_SEED)))
    rng = np.random.RandomState(seed)
    t_end = time.time() + budget
    it = done = 0
    ran = {k: 0 for k in dsoak.KERNELS}
    gmc = dict(compensated=0, compensated_with_centres=0, found_not_applied=0)
    blobs = {k: dict(multi=0, flag_off=0, flag_kept=0, masked=0, behind=0) for k in ("blobs", "gmc_blobs")}
    dirs = {"dir": dict(flag_off=0, per_stream=0), "lanes": dict(flag_off=0, per_stream=0, unstaged=0)}
    while time.time() < t_end:
        it += 1
        d = dsoak.draw(rng, it, seed)
        if not d["creatable"]:
            continue
        p = d["params"]
        where = (f"seed {seed} iteration {it} grid {p.grid_w}x{p.grid_h} {(d['w'], d['h'], d['kw'])} compact {d['compact']} "
                 f"window {d['window']}")
        s = gpu_scanner_factory(p)
        try:
            reached = check_draw(s, d, where)
        except (AssertionError, m.MtgpuError, pytest.fail.Exception) as e:
            raise AssertionError(f"{where} (derived_soak.replay({seed}, {it}) rebuilds the inputs): {e}") from e
        finally:
            s.close()
        done += 1
        for k in dsoak.KERNELS:
            ran[k] += d["support"][k]
        for k in gmc:
            gmc[k] += reached["gmc"] is not None and reached["gmc"][k] > 0
        for kernel, n in blobs.items():
            for k in n:
                n[k] += reached[kernel] is not None and reached[kernel][k] > 0
        for kernel, n in dirs.items():
            for k in n:
                n[k] += reached[kernel] is not None and reached[kernel][k] > 0
    # The budget is looked at between draws: a run overshoots it by at most one draw.  The costliest draw — the oracle on
    # 64 settings of 64 frames of 8000 records repeated 3.5 times, about 10^8 record visits on eight threads, and the numpy
    # models on 64 frames — takes about two seconds of CPU time, the average one a tenth of a second.  A second draw
    # starts whenever the first one ends inside the budget, so four seconds hold at least two; fewer means that the
    # expected values, not the kernels, have become the cost.  The blob scans' expected values label every frame's centre
    # plane by flood fill in plain Python; derived_soak.blob_batch labels each DISTINCT plane of a draw once, which keeps a
    # vectors_needed 0 draw (64 frames, one blob of up to 37 000 cells per stream) at the cost of its streams.  The direction
    # scan, the plane scan and the flow map add two numpy models and one oracle pass on the records as they are: a fifth
    # of a second on the costliest draw (docs/rounds/r27_direction_limits.md).
    assert done >= (2 if budget >= 4 else 1), f"only {done} configurations in {budget:.0f} s"
    print(f"derived soak: {done} random configurations checked in {budget:.0f} s, kernels run {ran}, the compensated scan's "
          f"draws with a frame compensated / one that keeps centres / a mode found and not applied: {gmc}, the blob scans' draws "
          f"with several blobs in a frame / a flag min_blob_cells turns off / one it keeps / masks / a frame behind the last stream: {blobs}, "
          f"the direction and plane scans' draws with a flag the byte or plane turns off / in the per-stream form / unstaged: {dirs}")
