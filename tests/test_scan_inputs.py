"""CPU tier: the inputs of the GPU parity tests say something about COUNTING.

GPU-vs-oracle parity of the scan is asserted on the per-frame centre count (tests/scan_checks.py).  That only bites on
frames that hold centres, so the inputs of test_scan_edge_configs are checked here, with the oracle alone: a later
change of synth.random_frames, or a new parameter set, cannot quietly leave a set with nothing to count."""
import numpy as np

import oracle_binding as ob
from np_model import check_frame_np
from scan_checks import EDGE_CFGS, EDGE_CFGS_WITHOUT_CENTRES, PLANTED, edge_config_inputs


def test_edge_config_inputs_hold_centres_to_count():
    assert len(EDGE_CFGS) == 31
    exempt = [cfg for cfg, reason in EDGE_CFGS_WITHOUT_CENTRES if reason]
    assert len(exempt) <= 6 and all(cfg in EDGE_CFGS for cfg in exempt)          # the list does not grow
    nonzero_frames, values = 0, set()
    for (w, h, kw) in EDGE_CFGS:
        p = ob.params_from_config(w, h, **kw)
        mv, off, sd, planted = edge_config_inputs(w, h, kw)
        assert len(off) == 49 + len(planted) and len(mv) == int(off[-1]) and len(sd) == len(off) - 1
        flags, centres = ob.scan_centres(p, mv, off, sd, nthreads=4)
        nz = int((centres > 0).sum())
        print((w, h, kw), "frames with centres", nz, "different counts", len(set(centres.tolist())))
        nonzero_frames += nz
        values |= set(centres[centres > 0].tolist())
        if (w, h, kw) in exempt:
            continue
        assert nz >= 10, ((w, h, kw), nz, "of", len(centres), "frames hold a centre: this set tests no counting")
    assert nonzero_frames >= 600 and len(values) >= 50, (nonzero_frames, len(values))


def test_planted_frames_have_the_counts_derived_by_hand():
    """The frames planted behind the random ones (VECTORS_NEEDED 255; 32767 x 40 with row bands): the oracle and the
    independent numpy model both give the count written down next to each frame's construction; at least 10 frames
    with centres and 4 different counts per set; the 48 random frames in front are the ones drawn before."""
    import zlib
    from mvtrim_amd import synth
    assert len(PLANTED) == 2
    for (w, h, kw), _ in PLANTED:
        assert (w, h, kw) in EDGE_CFGS
        p = ob.params_from_config(w, h, **kw)
        mv, off, sd, hand = edge_config_inputs(w, h, kw)
        flags, centres = ob.scan_centres(p, mv, off, sd)
        assert not centres[:48].any()                     # why frames are planted here at all
        assert centres[48:].tolist() == hand, (kw, centres[48:].tolist(), hand)
        assert sum(1 for c in hand if c) >= 10 and len(set(hand)) >= 4
        assert flags[48:].tolist() == [int(c >= max(1, p.clusters_needed)) for c in hand]
        for f in range(48, len(off) - 1):
            assert check_frame_np(p, mv[int(off[f]):int(off[f + 1])], True)[1] == hand[f - 48], f
        rng = np.random.RandomState(zlib.crc32(repr((w, h, sorted(kw.items()))).encode()) % (2 ** 31))
        mv0, off0, sd0 = synth.random_frames(rng, 48, 3000, w, h)
        assert np.array_equal(off[:49], off0) and np.array_equal(sd[:48], sd0)
        for name in ("dst_x", "dst_y", "src_x", "src_y"):
            assert np.array_equal(mv[name][:len(mv0)], mv0[name])
