"""The argument ladders of the derived scans' entry points, as a table: which check answers first, and with what text.

Every `_device` and host form of sweep, activity, zones, blobs, gmc, gmc_blobs and dir is called with a NULL context and
with arguments that break one rung, or two rungs at once; (rc, mtgpu_last_error()) then shows which of the two stands
first in the ladder.  All rungs ahead of "ctx is NULL" are reachable this way: no GPU and no mtgpu_create are needed.
(The rungs behind the context are held by each feature's GPU tests.)

A base call breaks nothing but the context.  Each entry of `breaks` changes the arguments so that ONE more rung fails;
the cases are every single break and every pair of breaks that do not touch the same argument — a superset of the
adjacent pairs.  The device forms never read through a pointer ahead of the context, so they get made-up addresses; the
host forms read frame_off and stream_off and get real arrays.

    python tests/api_arg_rungs.py --record --commit <id>     writes tests/golden/api_arg_rungs.json

records the answers of the library MTGPU_LIBRARY names (default: this tree's).  The fixture is recorded from a build of
the commit BEFORE a change to the ladders' code, never from the change itself; tests/test_api_arg_rungs_host.py only
compares.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "api_arg_rungs.json")

# ---- arguments

D = 0x7f0000010000                      # made-up device addresses, 64 KiB apart, never read
D_REC, D_OFF, D_SOFF, D_KEEP, D_FL, D_CEN, D_ALL, D_BL, D_LG, D_BOX, D_INFO, D_ROSE, D_ALLOW, D_ACT, D_FR = (D + (i << 16) for i in range(15))

_keepalive = []


def host(values, dtype):
    a = np.ascontiguousarray(values, dtype=dtype)
    _keepalive.append(a)
    return a.ctypes.data


OFF = host([0, 2, 4], np.uint64)          # two frames of two records
OFF_BACK = host([0, 5, 3], np.uint64)     # frame 1 ends before it begins
MV = host(np.zeros(4 * 40, np.uint8), np.uint8)
SOFF = host([0, 2], np.uint64)            # one stream, both frames
SOFF_SHORT = host([0, 1], np.uint64)      # one stream that ends at frame 1, not 2
SOFF_BACK = host([0, 2, 1], np.uint64)    # two streams, the second runs backwards
KEEP = host(np.zeros(64, np.uint64), np.uint64)
ALLOWS = host([255, 255], np.uint8)
OUT = [host(np.zeros(64, np.uint64), np.uint64) for _ in range(6)]

REC_BYTES = ("rec_bytes", dict(rec_bytes=7))


def device_rec_breaks():
    return [("d_rec_null", dict(d_rec=None)), ("compact_misaligned", dict(rec_bytes=8, d_rec=D_REC + 4)),
            ("d_rec_misaligned", dict(d_rec=D_REC + 2))]


def misaligned(names_and_bases, by):
    return [(f"{n}_misaligned", {n: b + by}) for n, b in names_and_bases]


def stream_table_breaks(soff, keep):
    """blobs, gmc_blobs: a keep mask comes with its stream table or not at all."""
    return [("stream_off_null_with_keep", {soff: None}), ("n_streams_0_with_keep", dict(n_streams=0)),
            ("keep_null_with_stream_off", {keep: None}), ("keep_null_with_n_streams", {keep: None, soff: None})]


def allow_table_breaks(soff, allows):
    return [("allow_given_stream_off_null", {soff: None}), ("allow_given_n_streams_0", dict(n_streams=0)),
            ("stream_off_given_allow_null", {allows: None}), ("n_streams_given_allow_null", {allows: None, soff: None})]


HOST_OFF_BREAKS = [("frame_off_backwards", dict(frame_off=OFF_BACK))]
HOST_STREAM_BREAKS = [("stream_off_backwards", dict(stream_off=SOFF_BACK, n_streams=2)), ("stream_off_short", dict(stream_off=SOFF_SHORT))]
HOST_MV_BREAK = [("mv_null_with_records", dict(mv=None))]
GMC_BREAKS = [("max_shift", dict(max_shift=200)), ("min_share_q8", dict(min_share_q8=300))]


def none_of(*names):
    return ("no_outputs", {n: None for n in names})


# entry point -> (parameter names in the order of the C signature, the base call, the breaks in the order of the ladder)
TABLE = {
    # the sweep and the activity map ask for the context FIRST: with a NULL context every call gives that answer
    "mtgpu_scan_sweep_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames thresholds n_thresholds vectors n_vectors d_centres stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, thresholds=None,
             n_thresholds=1, vectors=None, n_vectors=1, d_centres=D_CEN, stream=None),
        [REC_BYTES, ("n_thresholds", dict(n_thresholds=0)), ("d_centres_null", dict(d_centres=None))]),
    "mtgpu_scan_frames_sweep": (
        "c mv frame_off has_sd n_frames thresholds n_thresholds vectors n_vectors centres",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, thresholds=None, n_thresholds=1, vectors=None, n_vectors=1,
             centres=OUT[0]),
        [("n_thresholds", dict(n_thresholds=0)), ("centres_null", dict(centres=None))] + HOST_OFF_BREAKS),
    "mtgpu_activity_map_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames d_stream_off n_streams min_centres run_frames d_active d_centre "
        "d_frames stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, d_stream_off=D_SOFF,
             n_streams=1, min_centres=1, run_frames=0, d_active=D_ACT, d_centre=D_CEN, d_frames=D_FR, stream=None),
        [REC_BYTES, none_of("d_active", "d_centre", "d_frames"), ("d_frame_off_null", dict(d_frame_off=None))]),
    "mtgpu_activity_map": (
        "c mv frame_off has_sd n_frames stream_off n_streams min_centres active centre frames",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, stream_off=SOFF, n_streams=1, min_centres=1, active=OUT[0],
             centre=OUT[1], frames=OUT[2]),
        [none_of("active", "centre", "frames"), ("stream_off_null", dict(stream_off=None))] + HOST_OFF_BREAKS),
    "mtgpu_scan_zones_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames d_stream_off n_streams d_keep d_flags d_centres d_centres_all stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, d_stream_off=D_SOFF,
             n_streams=1, d_keep=D_KEEP, d_flags=D_FL, d_centres=D_CEN, d_centres_all=D_ALL, stream=None),
        [REC_BYTES, none_of("d_flags", "d_centres", "d_centres_all"), ("d_frame_off_null", dict(d_frame_off=None)),
         ("n_streams_0", dict(n_streams=0)), ("d_stream_off_null", dict(d_stream_off=None)), ("d_keep_null", dict(d_keep=None))] +
        misaligned([("d_frame_off", D_OFF), ("d_stream_off", D_SOFF), ("d_keep", D_KEEP)], 4) + device_rec_breaks() +
        misaligned([("d_centres", D_CEN), ("d_centres_all", D_ALL)], 2)),
    "mtgpu_scan_frames_zones": (
        "c mv frame_off has_sd n_frames stream_off n_streams keep flags centres centres_all",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, stream_off=SOFF, n_streams=1, keep=KEEP, flags=OUT[0],
             centres=OUT[1], centres_all=OUT[2]),
        [none_of("flags", "centres", "centres_all"), ("stream_off_null", dict(stream_off=None)), ("frame_off_null", dict(frame_off=None)),
         ("n_streams_0", dict(n_streams=0)), ("keep_null", dict(keep=None))] + HOST_OFF_BREAKS + HOST_STREAM_BREAKS + HOST_MV_BREAK),
    "mtgpu_scan_blobs_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames d_stream_off n_streams d_keep min_blob_cells d_flags d_centres "
        "d_blobs d_largest d_box stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, d_stream_off=D_SOFF,
             n_streams=1, d_keep=D_KEEP, min_blob_cells=1, d_flags=D_FL, d_centres=D_CEN, d_blobs=D_BL, d_largest=D_LG, d_box=D_BOX,
             stream=None),
        [REC_BYTES, none_of("d_flags", "d_centres", "d_blobs", "d_largest", "d_box"), ("d_frame_off_null", dict(d_frame_off=None))] +
        stream_table_breaks("d_stream_off", "d_keep") +
        misaligned([("d_frame_off", D_OFF), ("d_stream_off", D_SOFF), ("d_keep", D_KEEP)], 4) + device_rec_breaks() +
        misaligned([("d_centres", D_CEN), ("d_blobs", D_BL), ("d_largest", D_LG)], 2) + misaligned([("d_box", D_BOX)], 1)),
    "mtgpu_scan_frames_blobs": (
        "c mv frame_off has_sd n_frames stream_off n_streams keep min_blob_cells flags centres blobs largest box",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, stream_off=SOFF, n_streams=1, keep=KEEP, min_blob_cells=1,
             flags=OUT[0], centres=OUT[1], blobs=OUT[2], largest=OUT[3], box=OUT[4]),
        [none_of("flags", "centres", "blobs", "largest", "box"), ("frame_off_null", dict(frame_off=None))] +
        stream_table_breaks("stream_off", "keep") + HOST_OFF_BREAKS + HOST_STREAM_BREAKS + HOST_MV_BREAK),
    "mtgpu_scan_gmc_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames max_shift min_share_q8 d_flags d_centres d_info stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, max_shift=8,
             min_share_q8=128, d_flags=D_FL, d_centres=D_CEN, d_info=D_INFO, stream=None),
        [REC_BYTES] + GMC_BREAKS + [none_of("d_flags", "d_centres", "d_info"), ("d_frame_off_null", dict(d_frame_off=None))] +
        misaligned([("d_frame_off", D_OFF)], 4) + device_rec_breaks() + misaligned([("d_centres", D_CEN), ("d_info", D_INFO)], 2)),
    "mtgpu_scan_frames_gmc": (
        "c mv frame_off has_sd n_frames max_shift min_share_q8 flags centres info",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, max_shift=8, min_share_q8=128, flags=OUT[0], centres=OUT[1],
             info=OUT[2]),
        GMC_BREAKS + [none_of("flags", "centres", "info"), ("frame_off_null", dict(frame_off=None))] + HOST_OFF_BREAKS + HOST_MV_BREAK),
    "mtgpu_scan_gmc_blobs_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames d_stream_off n_streams d_keep max_shift min_share_q8 "
        "min_blob_cells d_flags d_centres d_blobs d_largest d_box d_info stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, d_stream_off=D_SOFF,
             n_streams=1, d_keep=D_KEEP, max_shift=8, min_share_q8=128, min_blob_cells=1, d_flags=D_FL, d_centres=D_CEN, d_blobs=D_BL,
             d_largest=D_LG, d_box=D_BOX, d_info=D_INFO, stream=None),
        [REC_BYTES] + GMC_BREAKS +
        [none_of("d_flags", "d_centres", "d_blobs", "d_largest", "d_box", "d_info"), ("d_frame_off_null", dict(d_frame_off=None))] +
        stream_table_breaks("d_stream_off", "d_keep") +
        misaligned([("d_frame_off", D_OFF), ("d_stream_off", D_SOFF), ("d_keep", D_KEEP)], 4) + device_rec_breaks() +
        misaligned([("d_centres", D_CEN), ("d_blobs", D_BL), ("d_largest", D_LG)], 2) + misaligned([("d_box", D_BOX)], 1) +
        misaligned([("d_info", D_INFO)], 2)),
    "mtgpu_scan_frames_gmc_blobs": (
        "c mv frame_off has_sd n_frames stream_off n_streams keep max_shift min_share_q8 min_blob_cells flags centres blobs largest "
        "box info",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, stream_off=SOFF, n_streams=1, keep=KEEP, max_shift=8,
             min_share_q8=128, min_blob_cells=1, flags=OUT[0], centres=OUT[1], blobs=OUT[2], largest=OUT[3], box=OUT[4], info=OUT[5]),
        GMC_BREAKS + [none_of("flags", "centres", "blobs", "largest", "box", "info"), ("frame_off_null", dict(frame_off=None))] +
        stream_table_breaks("stream_off", "keep") + HOST_OFF_BREAKS + HOST_STREAM_BREAKS + HOST_MV_BREAK),
    "mtgpu_scan_dir_device": (
        "c d_rec rec_bytes n_records d_frame_off d_has_sd n_frames d_stream_off n_streams d_allow allow d_flags d_centres d_rose stream",
        dict(c=None, d_rec=D_REC, rec_bytes=40, n_records=4, d_frame_off=D_OFF, d_has_sd=None, n_frames=2, d_stream_off=D_SOFF,
             n_streams=1, d_allow=D_ALLOW, allow=255, d_flags=D_FL, d_centres=D_CEN, d_rose=D_ROSE, stream=None),
        [("allow", dict(allow=300)), REC_BYTES, none_of("d_flags", "d_centres", "d_rose"), ("d_frame_off_null", dict(d_frame_off=None))] +
        allow_table_breaks("d_stream_off", "d_allow") + misaligned([("d_frame_off", D_OFF), ("d_stream_off", D_SOFF)], 4) +
        device_rec_breaks()[1:] + misaligned([("d_centres", D_CEN), ("d_rose", D_ROSE)], 2) + device_rec_breaks()[:1]),
    "mtgpu_scan_frames_dir": (
        "c mv frame_off has_sd n_frames stream_off n_streams allows allow flags centres rose",
        dict(c=None, mv=MV, frame_off=OFF, has_sd=None, n_frames=2, stream_off=SOFF, n_streams=1, allows=ALLOWS, allow=255,
             flags=OUT[0], centres=OUT[1], rose=OUT[2]),
        [("allow", dict(allow=300)), none_of("flags", "centres", "rose"), ("frame_off_null", dict(frame_off=None))] +
        allow_table_breaks("stream_off", "allows") + misaligned([("frame_off", OFF), ("stream_off", SOFF)], 4) +
        misaligned([("mv", MV)], 2) + misaligned([("centres", OUT[1]), ("rose", OUT[2])], 2) + HOST_OFF_BREAKS + HOST_STREAM_BREAKS +
        HOST_MV_BREAK),
}


def cases_of(entry):
    """[(case id, keyword arguments)]: the base call, every break, every pair of breaks on different arguments."""
    _, base, breaks = TABLE[entry]
    out = [("base", dict(base))]
    for label, change in breaks:
        out.append((label, dict(base, **change)))
    for (la, ca), (lb, cb) in itertools.combinations(breaks, 2):
        if not set(ca) & set(cb):
            out.append((f"{la}+{lb}", dict(base, **ca, **cb)))
    return out


def answers(lib, entry):
    """{case id: [rc, text]} of one entry point."""
    names = TABLE[entry][0].split()
    fn = getattr(lib, entry)
    got = {}
    for case, kw in cases_of(entry):
        assert sorted(kw) == sorted(names), (entry, case)
        rc = fn(*[kw[n] for n in names])
        got[case] = [int(rc), lib.mtgpu_last_error().decode("utf-8", "replace")]
    return got


def record(commit):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import mvtrim_amd as m
    lib = m.load_library()
    doc = {"recorded_from": commit,
           "how": "python tests/api_arg_rungs.py --record --commit <id>, with MTGPU_LIBRARY naming libmtgpu.so built from that commit",
           "answers": {entry: answers(lib, entry) for entry in TABLE}}
    with open(FIXTURE, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", sum(len(v) for v in doc["answers"].values()), "answers of", len(TABLE), "entry points from", commit)


if __name__ == "__main__":
    if "--record" not in sys.argv or "--commit" not in sys.argv:
        raise SystemExit(__doc__)
    record(sys.argv[sys.argv.index("--commit") + 1])
