"""GPU tier (`-m gpu`): the three labelling kernels on random and adversarial centre planes (tests/blob_planes.py) — the
resident blob scan and its pipe form (both csrc/blobs_kernels.hip) and the compensated blob scan
(csrc/gmc_blobs_kernels.hip), all three on the ONE text of the five passes in csrc/blob_label.h — against the flood-fill model (tests/blobs_model.py; tests/test_blob_planes_host.py holds it to
scipy on every plane).  This is where `unite`, the one place whose result depends on how the waves of a workgroup
interleave, meets percolation clusters, mazes, combs, bars and ties.

Every comparison is exact; there is no tolerance anywhere.  Outputs are pre-filled with junk.  One batch per test, the
cases ordered from the smallest grid to the largest: `unite` and `find_root` have no iteration cap, so a labelling bug
may hang instead of answering, and a time limit then points at one grid."""
import contextlib

import numpy as np
import pytest

import mvtrim_amd as m

import blob_planes as bp
import blobs_model as bm
import test_gpu_blobs as tb
import test_gpu_gmc_blobs as tg
from scan_checks import device_centres_of, to_device
from test_gpu_pipe_blobs import run

pytestmark = pytest.mark.gpu

PIPE_ORDER = [n for n in bp.GPU_ORDER if n != "240x135-m6-masked"]      # a pipe carries one keep plane: one masked batch does


def masks(b):
    return (None, None) if b.keeps is None else (tb.soff_tensor(b.soff), tb.keep_tensor(b.keeps))


def layout_name(compact):
    return "compact" if compact else "40-byte"


def blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep):
    """mtgpu_scan_blobs_device at min_blob_cells 1 into junk-filled outputs -> the five tensors."""
    import torch
    out = tb.junk_outputs(d_off.numel() - 1)
    torch.cuda.synchronize()
    res = s.scan_blobs_device(d_rec, d_off, d_sd, 1, d_soff, d_keep, compact=compact, want=tb.OUTPUTS, out=out)
    torch.cuda.synchronize()
    return res


def gmc_blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep, max_shift):
    """mtgpu_scan_gmc_blobs_device at min_blob_cells 1 into junk-filled outputs -> the six tensors."""
    import torch
    out = tg.junk_outputs(d_off.numel() - 1)
    torch.cuda.synchronize()
    res = s.scan_gmc_blobs_device(d_rec, d_off, d_sd, max_shift, bp.MIN_SHARE_Q8, 1, d_soff, d_keep, compact=compact, want=tg.OUTPUTS, out=out)
    torch.cuda.synchronize()
    return res


# ------------------------------------------------------------------ 1. the resident blob scan

@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_resident_blob_scan(gpu_scanner_factory, name):
    """mtgpu_scan_blobs_device on 40-byte and on compact records: flags, centres, blobs, largest and box are the
    model's; centres are also mtgpu_scan_centres_device's (mtgpu_scan_zones_device's under the masks)."""
    b, want = bp.batch(name), bp.expected(name)
    s = gpu_scanner_factory(b.p)
    d_soff, d_keep = masks(b)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(b.mv, b.off, b.sd, compact)
        label = f"{name}, blob scan, {layout_name(compact)}"
        got = tb.to_host(blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep))
        tb.assert_outputs(got, want, label, b.p, 1)
        tb.assert_identities(got, label)
        if b.keeps is None:
            _, scan_c = device_centres_of(s, d_rec, d_off, d_sd, compact)
        else:
            _, ce, _ = s.scan_zones_device(d_rec, d_off, d_sd, d_soff, d_keep, compact=compact)
            scan_c = ce.cpu().numpy().view(np.uint32)
        assert got["centres"].tolist() == scan_c.tolist(), label


# ------------------------------------------------------------------ 2. the pipe form

@pytest.mark.parametrize("name", PIPE_ORDER)
def test_pipe_form(gpu_scanner_factory, name):
    """The same frames through a ScanPipe with set_blobs(k, "largest") and set_blobs(k, "centres"), k the median of the
    model's `largest` over the batch: flags and the reported count are the model's, in tag order, zero-copy compact and
    copied 40-byte records.  The masked batch: its second stream through a pipe that carries that stream's keep plane."""
    b, want = bp.batch(name), bp.expected(name)
    lo, keep = (len(b.sd) // 2, b.keeps[1]) if b.keeps is not None else (0, None)
    frames = bp.pipe_frames(b, lo)
    centres, largest = want["centres"][lo:], want["largest"][lo:]
    k = max(1, int(np.median(largest)))
    flags = bm.flags_np(b.p, centres, largest, k).tolist()
    assert 0 < sum(flags) < len(flags)                       # the flag splits the frames
    s = gpu_scanner_factory(b.p)
    for layout in (m.LAYOUT_COMPACT8 | m.LAYOUT_ZERO_COPY, m.LAYOUT_AOS40):
        with contextlib.closing(m.ScanPipe(s, 1 << 15, 8, 2, layout=layout, centres=True)) as pipe:
            if keep is not None:
                pipe.set_keep(keep)
            pipe.set_blobs(k, "largest")
            assert run(pipe, frames) == (flags, largest.tolist()), (name, layout, "largest")
            pipe.set_blobs(k, "centres")
            assert run(pipe, frames) == (flags, centres.tolist()), (name, layout, "centres")


# ------------------------------------------------------------------ 3. consequence A, and the two kernels side by side

@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_compensated_blob_scan_at_max_shift_0(gpu_scanner_factory, name):
    """mtgpu_scan_gmc_blobs_device with max_shift 0: no pan, the five blob outputs are the model's — and, tensor for
    tensor, mtgpu_scan_blobs_device's.  Each kernel is held to the model first, so a failure names the one that left it."""
    import torch
    b, want = bp.batch(name), bp.expected(name)
    s = gpu_scanner_factory(b.p)
    d_soff, d_keep = masks(b)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(b.mv, b.off, b.sd, compact)
        ref = blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep)
        got = gmc_blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep, 0)
        tb.assert_outputs(tb.to_host(ref), want, f"{name}, blob scan (blobs_kernels.hip), {layout_name(compact)}", b.p, 1)
        host = tg.to_host(got)
        tg.assert_blobs(host, want, f"{name}, compensated blob scan at max_shift 0 (gmc_blobs_kernels.hip), {layout_name(compact)}", b.p, 1)
        assert not host["info"][:, :4].any(), name
        for k in tg.BLOB_OUTPUTS:
            assert ref[k].dtype == got[k].dtype and torch.equal(ref[k], got[k]), (name, layout_name(compact), k)


# ------------------------------------------------------------------ 4. the compensated blob scan under a pan

@pytest.mark.parametrize("name", bp.GPU_ORDER)
def test_compensated_blob_scan_under_a_pan(gpu_scanner_factory, name):
    """The batch under gmc_blobs_inputs.embed with the pan (9, -3), max_shift 16, min_share_q8 128: all six outputs are
    gmc_blobs_inputs.model_batch's and info reports the pan on every frame with side data — blob_label.h's passes on the
    residual plane, the same connectivity reached through the other kernel."""
    b, e, want = bp.batch(name), bp.embedded(name), bp.expected_embedded(name)
    assert e is not None
    s = gpu_scanner_factory(b.p)
    d_soff, d_keep = masks(b)
    has = np.flatnonzero(b.sd)
    for compact in (False, True):
        d_rec, d_off, d_sd = to_device(e.mv, e.off, b.sd, compact)
        label = f"{name} under {e.pan}, {layout_name(compact)}"
        got = tg.to_host(gmc_blob_scan(s, d_rec, d_off, d_sd, compact, d_soff, d_keep, bp.MAX_SHIFT))
        tg.assert_blobs(got, want, label, b.p, 1)
        tg.assert_info(got, want["info"], label)
        assert (got["info"][has][:, :2] == e.pan).all(), label
