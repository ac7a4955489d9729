"""GPU tier (`-m gpu`): the pipe forms of the masked scan, the blob scan and the compensated scan — zones_frames_kernel,
blobs_frames_kernel and gmc_frames_kernel with PIPE = true, launched from mtgpu_pipe_submit after mtgpu_pipe_set_keep,
mtgpu_pipe_set_blobs and mtgpu_pipe_set_gmc — on the random grids of tests/derived_soak.py for MTGPU_SOAK_SECONDS
(default 4 s; set it to minutes to hunt rare faults) and on five fixed grids with a word seam inside an analysed row.
Every draw gets a pipe round of its own (tests/pipe_soak.py: pipe geometry, frames as the pipe can express them, a record
copy in which the keep plane decides the vector, four keep planes), rebuilt on the CPU by pipe_soak.replay(seed, it).
Expected values: the oracle and the numpy models the repository already has (tests/test_pipe_soak_host.py holds their
sources against each other without a GPU).  Every comparison is exact; a setter whose preview says unsupported must
answer MT_ERR_UNSUPPORTED and leave the pipe as it was."""
import contextlib
import os
import time

import numpy as np
import pytest

import mvtrim_amd as m
from mvtrim_amd import _abi

import derived_soak as dsoak
import pipe_soak as ps

pytestmark = pytest.mark.gpu


def run(pipe, frames):
    """Feed, drain -> (flags, counts) lists; the tags must come back in submission order."""
    for i, f in enumerate(frames):
        pipe.feed(f, float(i), tag=i)
    out = pipe.drain_centres()
    assert [t for _, _, t, _ in out] == list(range(len(frames))), "tags are not in submission order"
    return [fl for _, fl, _, _ in out], [c for _, _, _, c in out]


def same(got, want, what):
    if got == want:
        return
    for name, g, w in (("flags", got[0], want[0]), ("counts", got[1], want[1])):
        bad = [i for i in range(max(len(g), len(w))) if i >= len(g) or i >= len(w) or g[i] != w[i]]
        if bad:
            f = bad[0]
            raise AssertionError(f"{what}: {name} differ on {len(bad)} of {len(w)} frames, first frame {f}: got "
                                 f"{g[f] if f < len(g) else None}, want {w[f] if f < len(w) else None}")


def refused(call, what):
    with pytest.raises(m.MtgpuError) as ei:
        call()
    assert ei.value.code == _abi.MT_ERR_UNSUPPORTED, (what, ei.value)


def check_round(pipe, d, r, keeps, blob_keeps, ran):
    """Steps 1 to 5 of a round in one pipe; every setting change comes after a drain (run() drains).  keeps: the planes of
    steps 2 and 4, blob_keeps: the planes of step 3.  ran: {form: count}, incremented for every form that ran."""
    sup, planes, fr, fg = r["support"], r["planes"], r["frames"], r["frames_gmc"]
    ms, q8, mb = r["max_shift"], r["share_q8"], r["min_blob_cells"]
    t_model = [0.0]

    def ex(form, keep=None):
        t0 = time.perf_counter()
        e = ps.expected_pipe(d, r, form, keep)
        t_model[0] += time.perf_counter() - t0
        return e

    def pair(e, count="centres"):
        return e["flags"], e[count]

    # 1. plain
    plain = pair(ex("plain"))
    assert pipe.has_keep is False and pipe.blobs is None and pipe.gmc() is None
    same(run(pipe, fr), plain, "plain")
    ran["plain"] += 1
    # 2. the masked scan
    if sup["masked"]:
        for k in keeps:
            pipe.set_keep(planes[k])
            assert pipe.has_keep
            same(run(pipe, fr), pair(ex("masked", k)), f"masked, plane {k}")
        pipe.set_keep(planes["ones"])
        same(run(pipe, fr), plain, "masked, all ones against plain")
        pipe.set_keep(None)
        ran["masked"] += 1
    else:
        refused(lambda: pipe.set_keep(planes["ones"]), "set_keep")
        assert not pipe.has_keep
        same(run(pipe, fr), plain, "plain after a refused set_keep")
    # 3. the blob scan under a plane, then without one
    for k in (list(blob_keeps) if sup["masked"] else []) + [None]:
        pipe.set_keep(None if k is None else planes[k])
        base = ex("plain") if k is None else ex("masked", k)
        if not sup["blobs"]:
            refused(lambda: pipe.set_blobs(max(mb, 1), "largest"), "set_blobs")
            assert pipe.blobs is None
            same(run(pipe, fr), pair(base), f"plane {k} after a refused set_blobs")
            continue
        for report in ("largest", "centres"):
            pipe.set_blobs(mb, report)
            if mb == 0:                                       # off: the masked or plain pipe
                assert pipe.blobs is None
                want = pair(base)
            else:
                assert pipe.blobs == (mb, report)
                want = pair(ex("blobs", k), report)
            same(run(pipe, fr), want, f"blobs min_blob_cells {mb} report {report}, plane {k}")
    ran["blobs"] += sup["blobs"] and mb > 0
    # 4. the compensated scan on pipe_mv
    pipe.set_blobs(0)
    pipe.set_keep(None)
    if sup["gmc"]:
        for k in [None] + ((list(keeps) + ["ones"]) if sup["masked"] else []):
            pipe.set_keep(None if k is None else planes[k])
            e = ex("gmc", None if k == "ones" else k)         # all ones must equal the run without a keep
            for report in ("vector", "centres"):
                pipe.set_gmc(ms, q8, report)
                assert pipe.gmc() == (ms, q8, report) and pipe.has_keep == (k is not None)
                got = run(pipe, fg)
                same(got, pair(e, report), f"gmc report {report}, plane {k}")
            if k is None:                                     # blobs and compensation: refused, nothing changes
                refused(lambda: pipe.set_blobs(mb or 3, "centres"), "set_blobs under set_gmc")
                assert pipe.blobs is None and pipe.gmc() == (ms, q8, "centres")
                same(run(pipe, fg), pair(e), "gmc after a refused set_blobs")
            if ms == 0:                                       # max_shift 0: the masked (or plain) pipe on the same records
                pipe.clear_gmc()
                same(run(pipe, fg), got, f"max_shift 0 against the pipe without compensation, plane {k}")
        if not sup["masked"]:
            refused(lambda: pipe.set_keep(planes["ones"]), "set_keep under set_gmc")
            assert not pipe.has_keep
        ran["gmc"] += 1
        ran["gmc_masked"] += sup["masked"]
    else:
        refused(lambda: pipe.set_gmc(ms, q8, "vector"), "set_gmc")
        assert pipe.gmc() is None
        same(run(pipe, fr), plain, "plain after a refused set_gmc")
    # 5. nothing is left behind
    pipe.clear_gmc()
    pipe.set_keep(None)
    assert pipe.has_keep is False and pipe.blobs is None and pipe.gmc() is None
    same(run(pipe, fr), plain, "plain, after every setting was taken back")
    return t_model[0]


def test_soak_pipe_forms(gpu_scanner_factory):
    budget = float(os.environ.get("MTGPU_SOAK_SECONDS", "4"))
    seed = int(os.environ.get("MTGPU_SOAK_SEED", str(dsoak.DEFAULT_SEED)))
    rng = np.random.RandomState(seed)
    t_end = time.time() + budget
    it = done = 0
    ran = dict(plain=0, masked=0, blobs=0, gmc=0, gmc_masked=0)
    reach = {}
    slowest = (0.0, 0.0, 0)
    while time.time() < t_end:
        it += 1
        d = dsoak.draw(rng, it, seed)
        if not d["creatable"]:
            continue
        t0 = time.perf_counter()
        r = ps.pipe_round(d, seed)
        p = d["params"]
        where = (f"seed {seed} iteration {it} grid {p.grid_w}x{p.grid_h} {(d['w'], d['h'], d['kw'])}, {ps.where_of(r)}")
        s = gpu_scanner_factory(p)
        try:
            with contextlib.closing(m.ScanPipe(s, r["max_records"], r["max_frames"], r["n_buffers"], layout=ps.layout_of(r))) as pipe:
                keeps = [k for k in ("left", "right", "drawn") if k in r["planes"]]
                t_model = check_round(pipe, d, r, keeps, [r["blob_plane"]], ran)
        except (AssertionError, m.MtgpuError, pytest.fail.Exception) as e:
            raise AssertionError(f"{where} (pipe_soak.replay({seed}, {it}) rebuilds the inputs): {e}") from e
        finally:
            s.close()
        done += 1
        took = time.perf_counter() - t0
        if took > slowest[0]:
            slowest = (took, t_model, it)
        for k, v in ps.reach(d, r).items():
            reach[k] = reach.get(k, 0) + bool(v)
    # The budget is looked at between draws: a run overshoots it by at most one draw.  The expected values of the costliest
    # draw take about a second of CPU time (pipe_soak's docstring), so four seconds hold at least two draws; fewer means
    # that the expected values, not the kernels, have become the cost.
    assert done >= (2 if budget >= 4 else 1), f"only {done} configurations in {budget:.0f} s"
    print(f"pipe soak: {done} random configurations checked in {budget:.0f} s; draws that ran each form {ran}; draws in which a "
          f"frame's masked vector differed from its unmasked one: {reach.get('vector_masked', 0)}; reach {reach}; slowest draw: "
          f"iteration {slowest[2]}, {slowest[0]:.2f} s, of which the expected values took {slowest[1]:.2f} s "
          f"({100.0 * slowest[1] / max(slowest[0], 1e-9):.0f} %)")


def test_pipe_forms_on_word_seam_grids(gpu_scanner_factory):
    """The fixed complement of the soak: gw 63, 64, 65, 128 and 129 (W 1, 2 and 3), gh 17 under a margin of 2 (y_lo 2,
    crows 13 < R), the two pans split at column 64 (32 on the 63 columns), keep planes left and right of the split, of
    column 63, column 64 and the last column alone, each also with an analysed row cleared; compact8 + zero-copy and aos40
    with a device mirror.  Steps 1 to 5 of the soak against the models, and the unmasked compensated pipe against
    mtgpu_scan_frames_gmc on the same frames."""
    import pipe_gmc_inputs as pgi
    for width in ps.SEAM_WIDTHS:
        shared = None
        for compact, zero_copy in ps.SEAM_LAYOUTS:
            r = ps.seam_round(width, compact, zero_copy)
            if shared is not None:
                r["memo"] = shared                                # the expected values of a grid are computed once
            shared = r["memo"]
            p = r["params"]
            assert all(r["support"].values()), r["support"]
            s = gpu_scanner_factory(p)
            ran = dict(plain=0, masked=0, blobs=0, gmc=0, gmc_masked=0)
            keeps = [k for k in r["planes"] if k != "ones"]
            where = f"grid {p.grid_w}x{p.grid_h} margin {p.vertical_margin} compact {compact} zero-copy {zero_copy}"
            try:
                with contextlib.closing(m.ScanPipe(s, r["max_records"], r["max_frames"], r["n_buffers"], layout=ps.layout_of(r))) as pipe:
                    check_round(pipe, None, r, keeps, keeps, ran)
                    fl, ce, info = s.scan_gmc(m.FrameBatch.from_frames(list(r["frames_gmc"])), r["max_shift"], r["share_q8"])
                    vec = [pgi.pack_vector(x, y) for x, y in zip(info["gx"].tolist(), info["gy"].tolist())]
                    pipe.set_gmc(r["max_shift"], r["share_q8"], "centres")
                    same(run(pipe, r["frames_gmc"]), (fl.tolist(), ce.tolist()), "the compensated pipe against scan_gmc, centres")
                    pipe.set_gmc(r["max_shift"], r["share_q8"], "vector")
                    same(run(pipe, r["frames_gmc"]), (fl.tolist(), vec), "the compensated pipe against scan_gmc, vector")
            except (AssertionError, m.MtgpuError) as e:
                raise AssertionError(f"{where}: {e}") from e
            finally:
                s.close()
            assert ran == dict(plain=1, masked=1, blobs=1, gmc=1, gmc_masked=1), ran
