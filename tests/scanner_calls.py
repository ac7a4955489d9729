"""Call traces of scanner.py: what every wrapper hands to the library and what it returns, without a GPU and without
libmtgpu.so.  A MotionScanner / ScanPipe made through __new__ gets a recording stand-in for its library; the device
forms get CPU tensors and an explicit integer stream.  cases() lists the cases, run_case() replays one against a
scanner module, record() writes tests/golden/scanner_calls.json:

    python tests/scanner_calls.py --record path/to/scanner.py

records the golden from THAT file, loaded as a sibling of the package's modules (the golden of a refactor is recorded
from the scanner.py of the commit before it).  tests/test_scanner_calls_host.py replays every case on the tree's own
scanner.py and compares for equality."""
import ctypes as C
import importlib.util
import inspect
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "scanner_calls.json")

GRID = (4.0, 4, 2, 1, 2, 70, 9)          # ScanParams: 70 cells a row, wider than one keep word
GW, GH, KW = 70, 9, 2
CTX, PIPE, STREAM = 0x7001, 0x7002, 0x7003
_BYREF = type(C.byref(C.c_int()))


def load_scanner(path=None):
    """The package's scanner module, or the scanner.py at `path` loaded next to the package's other modules."""
    import mvtrim_amd
    if path is None:
        return mvtrim_amd.scanner
    spec = importlib.util.spec_from_file_location("mvtrim_amd._scanner_elsewhere", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def argtypes():
    """symbol -> argtypes, from every ABI* dict of _abi."""
    from mvtrim_amd import _abi
    out = {}
    for k, v in vars(_abi).items():
        if k.startswith("ABI") and isinstance(v, dict):
            out.update({name: args for name, (_, args) in v.items()})
    return out


class Recorder:
    """Stands in for the loaded library: every symbol is a function that notes (symbol, args) and answers 0, or what
    answers[symbol](args) says."""

    def __init__(self, answers=None):
        self.calls = []
        self.answers = answers or {}

    def __getattr__(self, symbol):
        if symbol.startswith("__"):
            raise AttributeError(symbol)

        def call(*args):
            self.calls.append((symbol, args))
            answer = self.answers.get(symbol)
            return 0 if answer is None else answer(args)
        return call


# ---------------------------------------------------------------- the normaliser
def _addresses(name, v, into):
    """Base address -> name, for every array and tensor reachable from a named value."""
    import torch
    if isinstance(v, np.ndarray):
        into.setdefault(v.ctypes.data, name)
    elif isinstance(v, torch.Tensor):
        if v.data_ptr():
            into.setdefault(v.data_ptr(), name)
    elif isinstance(v, dict):
        for k, x in v.items():
            _addresses(f"{name}.{k}", x, into)
    elif isinstance(v, (tuple, list)):
        for i, x in enumerate(v):
            _addresses(f"{name}[{i}]", x, into)
    elif hasattr(v, "frame_off") and hasattr(v, "mv"):
        for k in ("mv", "frame_off", "pts", "has_sd"):
            _addresses(f"{name}.{k}", getattr(v, k), into)


def _cvalue(obj):
    if isinstance(obj, C.Structure):
        return {n: _cvalue(getattr(obj, n)) for n, *_ in obj._fields_}
    if isinstance(obj, C.Array):
        return [_cvalue(x) for x in obj]
    return getattr(obj, "value", obj)


def _arg(a, ctype, names):
    if a is None:
        return None
    if isinstance(a, C.Array):
        return _cvalue(a)
    if isinstance(a, _BYREF):
        return {"byref": _cvalue(a._obj)}
    if isinstance(a, C.c_void_p):
        a, ctype = a.value, C.c_void_p
        if a is None:
            return None
    if isinstance(a, (bool, int, float)):
        if ctype is C.c_void_p:
            return 0 if a == 0 else names.get(a, "internal")
        return a
    return repr(a)


def _describe(x, inputs):
    import torch
    if isinstance(x, np.ndarray):
        return {"numpy": str(x.dtype), "shape": list(x.shape), "bytes": np.unique(x.view(np.uint8)).tolist()}
    if isinstance(x, torch.Tensor):
        d = {"torch": str(x.dtype), "shape": list(x.shape)}
        same = [k for k, v in inputs.items() if v is x]
        if same:
            d["is"] = same[0]
        return d
    if isinstance(x, dict):
        return {k: _describe(v, inputs) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return [_describe(v, inputs) for v in x]
    if isinstance(x, (np.integer, np.floating)):
        return x.item()
    return x


def _flat_inputs(bound):
    out = {}
    for k, v in bound.items():
        out[k] = v
        if isinstance(v, dict):
            out.update({f"{k}.{n}": x for n, x in v.items()})
        elif isinstance(v, tuple):
            out.update({f"{k}[{i}]": x for i, x in enumerate(v)})
    return out


def run_case(mod, case):
    """One case against the scanner module `mod` -> {"calls": [[symbol, args...]], "returns": ...} or {"calls", "raises"}."""
    target, method, build = case[1], case[2], case[3]
    args, kwargs, answers = build(mod)
    rec = Recorder(answers)
    params = mod.ScanParams(*GRID)
    scanner = mod.MotionScanner.__new__(mod.MotionScanner)
    scanner.params, scanner.device, scanner._lib, scanner._ctx = params, 0, rec, C.c_void_p(CTX)
    scanner._pipes = set()
    if target == "scanner":
        obj = scanner
    elif target == "pipe":
        obj = mod.ScanPipe.__new__(mod.ScanPipe)
        obj._lib, obj._scanner, obj._pipe = rec, scanner, C.c_void_p(PIPE)
    else:
        obj = mod
    attr = inspect.getattr_static(obj if target == "module" else type(obj), method)
    names = {CTX: "ctx", PIPE: "pipe", STREAM: "stream"}
    inputs = {}
    if not isinstance(attr, property):
        bound = inspect.signature(getattr(obj, method)).bind(*args, **kwargs).arguments
        inputs = _flat_inputs(bound)
        for k, v in bound.items():
            _addresses(k, v, names)
    loader = mod.load_library
    mod.load_library = lambda: rec
    try:
        try:
            ret = getattr(obj, method) if isinstance(attr, property) else getattr(obj, method)(*args, **kwargs)
            out = {"returns": None}
        except Exception as e:       # the wrappers' own refusals are part of the trace
            ret = None
            out = {"raises": [type(e).__name__, str(e)]}
    finally:
        mod.load_library = loader
    _addresses("ret", ret, names)
    if "returns" in out:
        out["returns"] = _describe(ret, inputs)
    types = argtypes()
    calls = []
    for symbol, a in rec.calls:
        assert len(a) == len(types[symbol]), f"{symbol}: {len(a)} arguments for {len(types[symbol])}"
        calls.append([symbol] + [_arg(x, t, names) for x, t in zip(a, types[symbol])])
    out["calls"] = calls
    return json.loads(json.dumps(out))


# ---------------------------------------------------------------- the inputs
OFFS = {0: [0], 1: [0, 0], 3: [0, 2, 2, 5]}            # F = 0; one frame without records; three frames, five records
SOFFS = {0: [0], 1: [0, 1], 3: [0, 2, 3]}              # ... in no, one and two streams
# name -> (torch dtype name, trailing shape) of the device outputs, as the docstrings of scanner.py give them
DEVICE_OUT = {"flags": ("uint8", ()), "centres": ("int32", ()), "blobs": ("int32", ()), "largest": ("int32", ()),
              "run": ("int32", ()), "pos": ("int32", ()), "rose": ("int32", (8,)), "box": ("int16", (4,)),
              "info": ("int32", (5,)), "active": ("int32", (GH, GW)), "centre": ("int32", (GH, GW)), "frames": ("int32", ())}


def batch(mod, F, sd=True):
    from mvtrim_amd import MV_DTYPE
    off = np.array(OFFS[F], dtype=np.uint64)
    return mod.FrameBatch(np.zeros(int(off[-1]), dtype=MV_DTYPE), off, None, np.ones(F, dtype=np.uint8) if sd else None)


def soff(F):
    return np.array(SOFFS[F], dtype=np.uint64)


def keep(F):
    return np.ones((len(SOFFS[F]) - 1, GH, KW), dtype=np.uint64)


def dbatch(F, sd=True, compact=False):
    import torch
    rec = torch.zeros(OFFS[F][-1] * (8 if compact else 40), dtype=torch.uint8)
    return rec, torch.tensor(OFFS[F], dtype=torch.int64), (torch.ones(F, dtype=torch.uint8) if sd else None)


def dsoff(F):
    import torch
    return torch.tensor(SOFFS[F], dtype=torch.int64)


def dkeep(F):
    import torch
    return torch.ones((len(SOFFS[F]) - 1, GH, KW), dtype=torch.int64)


class MergeParams:
    """Stands in a device case for a MergeParams of the module under test."""


def tensor(lead, name, dtype=None):
    import torch
    d, trail = DEVICE_OUT[name]
    return torch.zeros((lead,) + trail, dtype=getattr(torch, dtype or d))


# ---------------------------------------------------------------- the cases
def cases():
    """[(id, target, method, build)]: build(mod) -> (args, kwargs, answers), fresh inputs on every call."""
    import torch
    out = []

    def add(cid, method, build, target="scanner"):
        out.append((cid, target, method, build))

    def host(cid, method, fn):                        # fn(mod, F, sd) -> (args, kwargs)
        for F, sd in itertools.product((0, 1, 3), (0, 1)):
            add(f"{cid}/F{F}/sd{sd}", method, lambda mod, F=F, sd=sd: fn(mod, F, sd) + (None,))

    def dev(cid, method, fn, compacts=(0, 1)):         # fn(F, sd, compact) -> (args, kwargs); the stream is added
        for F, sd, c in itertools.product((0, 1, 3), (0, 1), compacts):
            def build(mod, F=F, sd=sd, c=c):
                a, k = fn(F, sd, c)
                a = tuple(mod.MergeParams(10.0, 1.0, 0.5, 5.0) if x is MergeParams else x for x in a)
                return a, dict(k, stream=STREAM), None
            add(f"{cid}/F{F}/sd{sd}/c{c}", method, build)

    def one(cid, method, fn, target="scanner", answers=None):     # fn(mod) -> (args, kwargs)
        add(cid, method, lambda mod: fn(mod) + (answers,), target)

    def done(cid, method, fn):                        # one device call at three frames; fn() -> (args, kwargs)
        def build(mod):
            a, k = fn()
            return a, dict(k, stream=STREAM), None
        add(cid, method, build)

    # ---- host forms on the grid of batches
    host("check_frames", "check_frames", lambda m, F, sd: ((batch(m, F, sd),), {}))
    host("count_centres", "count_centres", lambda m, F, sd: ((batch(m, F, sd),), {}))
    host("sweep_centres", "sweep_centres", lambda m, F, sd: ((batch(m, F, sd), [4.0, 9.0], [1, 2, 3]), {}))
    host("activity_map", "activity_map", lambda m, F, sd: ((batch(m, F, sd), soff(F)), {"min_centres": 2}))
    host("scan_zones", "scan_zones", lambda m, F, sd: ((batch(m, F, sd), soff(F), keep(F)), {}))
    host("scan_dir", "scan_dir", lambda m, F, sd: ((batch(m, F, sd), 0x0F), {}))
    host("scan_dir/streams", "scan_dir", lambda m, F, sd: ((batch(m, F, sd),), {
        "stream_off": soff(F), "allows": np.arange(len(SOFFS[F]) - 1, dtype=np.uint8)}))
    host("scan_lanes", "scan_lanes", lambda m, F, sd: ((batch(m, F, sd), np.full((GH, GW), 255, np.uint8)), {}))
    host("scan_lanes/streams", "scan_lanes", lambda m, F, sd: ((batch(m, F, sd), np.zeros((len(SOFFS[F]) - 1, GH, GW), np.uint8)),
                                                                {"stream_off": soff(F)}))
    host("flow_map", "flow_map", lambda m, F, sd: ((batch(m, F, sd), soff(F)), {}))
    host("scan_gmc", "scan_gmc", lambda m, F, sd: ((batch(m, F, sd),), {"max_shift": 5, "min_share_q8": 77}))
    host("scan_blobs", "scan_blobs", lambda m, F, sd: ((batch(m, F, sd), 3), {}))
    host("scan_blobs/keep", "scan_blobs", lambda m, F, sd: ((batch(m, F, sd),), {"stream_off": soff(F), "keep": keep(F)}))
    host("scan_gmc_blobs", "scan_gmc_blobs", lambda m, F, sd: ((batch(m, F, sd), 5, 77, 3), {}))
    host("scan_gmc_blobs/keep", "scan_gmc_blobs", lambda m, F, sd: ((batch(m, F, sd),), {"stream_off": soff(F), "keep": keep(F)}))
    host("motion_scalar", "motion_scalar", lambda m, F, sd: ((batch(m, F, sd), [0.5 * i for i in range(F)]), {}))
    host("persist", "persist", lambda m, F, sd: ((np.ones(F, np.uint8), soff(F)), {"has_sd": np.ones(F, np.uint8) if sd else None,
                                                                                 "min_run": 2, "max_dropout": 1, "reach": 3}))

    # ---- host forms: each method's own arguments, refusals and stream_off handling
    b3 = lambda m: batch(m, 3)        # noqa: E731
    one("check_frames/foreign_dtypes", "check_frames", lambda m: ((m.FrameBatch(batch(m, 3).mv, [0, 2, 2, 5], None, [1, 0, 1]),), {}))
    one("sweep_centres/no_settings", "sweep_centres", lambda m: ((b3(m), [], []), {}))
    one("sweep_centres/int32", "sweep_centres", lambda m: ((b3(m), [4.0], [2 ** 31]), {}))
    for w in [("active",), ("centre",), ("frames",), ("active", "centre", "frames"), (), ("frames", "rose")]:
        one("activity_map/want=" + ",".join(w), "activity_map", lambda m, w=w: ((b3(m), soff(3)), {"want": w}))
    one("scan_zones/want_all", "scan_zones", lambda m: ((b3(m), soff(3), keep(3)), {"want_all": True}))
    one("scan_zones/one_keep", "scan_zones", lambda m: ((b3(m), soff(3), np.ones((GH, KW), np.uint64)), {}))
    one("scan_zones/keep_shape", "scan_zones", lambda m: ((b3(m), soff(3), np.ones((2, GH, 1), np.uint64)), {}))
    empty = lambda: np.zeros(0, dtype=np.uint64)      # noqa: E731
    one("activity_map/no_stream_off", "activity_map", lambda m: ((batch(m, 0), empty()), {}))
    one("scan_zones/no_stream_off", "scan_zones", lambda m: ((batch(m, 0), empty(), np.ones((GH, KW), np.uint64)), {}))
    one("persist/no_stream_off", "persist", lambda m: ((np.zeros(0, np.uint8), empty()), {}))
    one("flow_map/no_stream_off", "flow_map", lambda m: ((batch(m, 0), empty()), {}))
    one("scan_dir/no_stream_off", "scan_dir", lambda m: ((batch(m, 0),), {"stream_off": empty(), "allows": np.zeros(0, np.uint8)}))
    one("scan_lanes/no_stream_off", "scan_lanes", lambda m: ((batch(m, 0), np.zeros((0, GH, GW), np.uint8)), {"stream_off": empty()}))
    one("scan_blobs/no_stream_off", "scan_blobs", lambda m: ((batch(m, 0),), {"stream_off": empty(), "keep": np.ones((GH, KW), np.uint64)}))
    one("scan_gmc_blobs/no_stream_off", "scan_gmc_blobs", lambda m: ((batch(m, 0),), {"stream_off": empty(), "keep": np.ones((GH, KW), np.uint64)}))
    one("scan_dir/alone:stream_off", "scan_dir", lambda m: ((b3(m),), {"stream_off": soff(3)}))
    one("scan_dir/alone:allows", "scan_dir", lambda m: ((b3(m),), {"allows": [1, 2]}))
    one("scan_dir/allows_count", "scan_dir", lambda m: ((b3(m),), {"stream_off": soff(3), "allows": [1, 2, 3]}))
    one("scan_dir/allows_range", "scan_dir", lambda m: ((b3(m),), {"stream_off": soff(3), "allows": [1, 256]}))
    one("scan_lanes/planes_shape", "scan_lanes", lambda m: ((b3(m), np.zeros((GH, GW + 1), np.uint8)), {}))
    one("scan_lanes/planes_shape_streams", "scan_lanes", lambda m: ((b3(m), np.zeros((GH, GW), np.uint8)), {"stream_off": soff(3)}))
    for meth in ("scan_blobs", "scan_gmc_blobs"):
        one(meth + "/alone:stream_off", meth, lambda m: ((b3(m),), {"stream_off": soff(3)}))
        one(meth + "/alone:keep", meth, lambda m: ((b3(m),), {"keep": keep(3)}))
        one(meth + "/keep_shape", meth, lambda m: ((b3(m),), {"stream_off": soff(3), "keep": np.ones((3, GH, KW), np.uint64)}))
        one(meth + "/one_keep", meth, lambda m: ((b3(m),), {"stream_off": soff(3), "keep": np.ones((GH, KW), np.uint64)}))
    one("motion_scalar/n_sec=0", "motion_scalar", lambda m: ((b3(m), [0.0, 1.5, None]), {"n_sec": 0}))
    one("motion_scalar/n_sec=4", "motion_scalar", lambda m: ((b3(m), [0.0, 1.5, None]), {"n_sec": 4}))
    one("motion_scalar/n_sec=-1", "motion_scalar", lambda m: ((b3(m), [0.0, 1.5, None]), {"n_sec": -1}))
    one("motion_scalar/all_null", "motion_scalar", lambda m: ((b3(m), [None, -2.0, float("nan")]), {}))
    one("motion_scalar/count", "motion_scalar", lambda m: ((b3(m), [0.0, 1.0]), {}))
    box = lambda n: np.zeros(n, dtype=np.dtype([("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2")]))     # noqa: E731
    one("persist/box", "persist", lambda m: ((np.ones(3, np.uint8), soff(3)), {"box": box(3)}))
    one("persist/box_count", "persist", lambda m: ((np.ones(3, np.uint8), soff(3)), {"box": box(2)}))
    one("persist/sd_count", "persist", lambda m: ((np.ones(3, np.uint8), soff(3)), {"has_sd": np.ones(4, np.uint8)}))
    one("merge_segments", "merge_segments", lambda m: (([0.5, 0.25, 3.0], m.MergeParams(10.0, 1.0, 0.5, 5.0)), {"job_semantics": True}))
    one("merge_segments/none", "merge_segments", lambda m: ((np.zeros(0), m.MergeParams(10.0, 1.0, 0.5, 5.0)), {"cap": 0}))
    one("plan", "plan", lambda m: ((), {}))
    one("stats", "stats", lambda m: ((), {}))

    # ---- the previews (module functions; the stand-in answers for load_library())
    for name in ("plan", "sweep", "activity", "zones", "blobs", "gmc", "gmc_blobs", "dir", "lanes"):
        extra = (3, 2) if name == "sweep" else ()
        one(name + "_preview", name + "_preview", lambda m, e=extra: ((m.ScanParams(*GRID),) + e, {}), "module")
        one(name + "_preview/lds", name + "_preview", lambda m, e=extra: ((m.ScanParams(*GRID),) + e, {"lds_bytes": 65536}), "module")
    one("plan_preview/cus", "plan_preview", lambda m: ((m.ScanParams(*GRID), 65536, 64), {}), "module")
    one("persist_preview", "persist_preview", lambda m: ((), {}), "module")

    # ---- device forms on the grid of batches
    dev("check_frames_device", "check_frames_device", lambda F, sd, c: (dbatch(F, sd), {}), (0,))
    dev("check_frames_device_compact", "check_frames_device_compact", lambda F, sd, c: (dbatch(F, sd, True), {}), (1,))
    dev("count_centres_device", "count_centres_device", lambda F, sd, c: (dbatch(F, sd, c), {"compact": bool(c)}))
    dev("sweep_centres_device", "sweep_centres_device", lambda F, sd, c: (dbatch(F, sd, c) + ([4.0, 9.0], [1, 2, 3]), {"compact": bool(c)}))
    dev("activity_map_device", "activity_map_device", lambda F, sd, c: (dbatch(F, sd, c) + (dsoff(F),), {
        "min_centres": 2, "run_frames": 4, "compact": bool(c)}))
    dev("scan_zones_device", "scan_zones_device", lambda F, sd, c: (dbatch(F, sd, c) + (dsoff(F), dkeep(F)), {"compact": bool(c)}))
    dev("scan_dir_device", "scan_dir_device", lambda F, sd, c: (dbatch(F, sd, c) + (0x0F,), {"compact": bool(c)}))
    dev("scan_dir_device/streams", "scan_dir_device", lambda F, sd, c: (dbatch(F, sd, c), {
        "d_stream_off": dsoff(F), "d_allow": torch.zeros(max(len(SOFFS[F]) - 1, 1), dtype=torch.uint8), "compact": bool(c)}))
    dev("scan_lanes_device", "scan_lanes_device", lambda F, sd, c: (dbatch(F, sd, c) + (torch.zeros((GH, GW), dtype=torch.uint8),),
                                                                    {"compact": bool(c)}))
    dev("scan_lanes_device/streams", "scan_lanes_device", lambda F, sd, c: (
        dbatch(F, sd, c) + (torch.zeros((max(len(SOFFS[F]) - 1, 1), GH, GW), dtype=torch.uint8),), {"d_stream_off": dsoff(F), "compact": bool(c)}))
    dev("flow_map_device", "flow_map_device", lambda F, sd, c: (dbatch(F, sd, c) + (dsoff(F),), {"compact": bool(c)}))
    dev("scan_gmc_device", "scan_gmc_device", lambda F, sd, c: (dbatch(F, sd, c) + (5, 77), {"compact": bool(c)}))
    dev("scan_blobs_device", "scan_blobs_device", lambda F, sd, c: (dbatch(F, sd, c) + (3,), {"compact": bool(c)}))
    dev("scan_blobs_device/keep", "scan_blobs_device", lambda F, sd, c: (dbatch(F, sd, c), {
        "d_stream_off": dsoff(F), "d_keep": dkeep(F), "compact": bool(c)}))
    dev("scan_gmc_blobs_device", "scan_gmc_blobs_device", lambda F, sd, c: (dbatch(F, sd, c) + (5, 77, 3), {"compact": bool(c)}))
    dev("scan_gmc_blobs_device/keep", "scan_gmc_blobs_device", lambda F, sd, c: (dbatch(F, sd, c), {
        "d_stream_off": dsoff(F), "d_keep": dkeep(F), "compact": bool(c)}))
    dev("persist_device", "persist_device", lambda F, sd, c: ((torch.ones(F, dtype=torch.uint8), dsoff(F)), {
        "d_has_sd": torch.ones(F, dtype=torch.uint8) if sd else None, "d_box": tensor(F, "box") if c else None,
        "min_run": 2, "max_dropout": 1, "reach": 3, "work": torch.zeros(F, dtype=torch.int32)}))
    dev("motion_scores_device", "motion_scores_device", lambda F, sd, c: (dbatch(F)[:2], {}), (0,))
    dev("motion_bins_device", "motion_bins_device", lambda F, sd, c: (
        (torch.zeros(F, dtype=torch.float64), torch.zeros(F, dtype=torch.int32) if sd else None, torch.zeros(F, dtype=torch.float64),
         dsoff(F), 4), {}), (0,))
    dev("flags_from_centres", "flags_from_centres", lambda F, sd, c: ((torch.zeros(F, dtype=torch.int32), 2), {}), (0,))
    dev("merge_streams_device", "merge_streams_device", lambda F, sd, c: (
        (torch.ones(F, dtype=torch.uint8) if sd else None, torch.zeros(F, dtype=torch.float64), dsoff(F),
         torch.zeros(32 * (len(SOFFS[F]) - 1), dtype=torch.uint8)),
        {"job_semantics": bool(c), "seg_cap": 8, "out": (torch.zeros((len(SOFFS[F]) - 1, 8, 2), dtype=torch.float64),
                                                         torch.zeros((len(SOFFS[F]) - 1, 40), dtype=torch.uint8),
                                                         torch.zeros(2 * F, dtype=torch.float64))}))
    dev("merge_timestamps_device", "merge_timestamps_device", lambda F, sd, c: (
        (torch.zeros(F, dtype=torch.float64), MergeParams), {"job_semantics": bool(c), "seg_cap": 8}))

    # ---- device forms: the None / False / True / tensor ladder of every optional output, at three frames
    ladder = {"none": lambda n, d: None, "false": lambda n, d: False, "true": lambda n, d: True,
              "tensor": lambda n, d: tensor(3, n), "short": lambda n, d: tensor(2, n), "dtype": lambda n, d: tensor(3, n, d)}
    wrong = {"flags": "int32", "centres": "uint8", "info": "int16"}
    for meth, args, names in (
            ("count_centres_device", lambda: dbatch(3), ("flags", "centres")),
            ("scan_zones_device", lambda: dbatch(3) + (dsoff(3), dkeep(3)), ("flags", "centres", "centres_all")),
            ("scan_gmc_device", lambda: dbatch(3), ("flags", "centres", "info"))):
        for n in names:
            for rung, make in ladder.items():
                table = "centres" if n == "centres_all" else n
                done(f"{meth}/{n}={rung}", meth, lambda a=args, n=n, t=table, make=make: (a(), {n: make(t, wrong[t])}))
        done(f"{meth}/all=false", meth, lambda a=args, names=names: (a(), {n: False for n in names}))
    # (a tensor of the wrong type at F = 0: the forms that return early do not look at it, the others do)
    done("count_centres_device/F0/flags=dtype", "count_centres_device", lambda: (dbatch(0), {"flags": tensor(0, "flags", "int32")}))
    done("count_centres_device/F0/centres=dtype", "count_centres_device", lambda: (dbatch(0), {"centres": tensor(0, "centres", "uint8")}))
    done("motion_scores_device/F0/terms=dtype", "motion_scores_device", lambda: (dbatch(0)[:2], {"terms": tensor(0, "centres", "uint8")}))
    done("scan_zones_device/F0/flags=dtype", "scan_zones_device", lambda: (dbatch(0) + (dsoff(0), dkeep(0)), {"flags": tensor(0, "flags", "int32")}))
    done("scan_gmc_device/F0/info=dtype", "scan_gmc_device", lambda: (dbatch(0), {"info": tensor(0, "info", "int16")}))
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)      # noqa: E731
    for rung, v in (("none", lambda: None), ("false", lambda: False), ("true", lambda: True), ("tensor", lambda: tensor(3, "flags")),
                    ("short", lambda: tensor(2, "flags")), ("dtype", lambda: tensor(3, "flags", "int32"))):
        done(f"check_frames_device/flags={rung}", "check_frames_device", lambda v=v: (dbatch(3), {"flags": v()}))
        done(f"check_frames_device_compact/flags={rung}", "check_frames_device_compact", lambda v=v: (dbatch(3, True, True), {"flags": v()}))
        done(f"flags_from_centres/flags={rung}", "flags_from_centres", lambda v=v: ((torch.zeros(3, dtype=torch.int32), 2), {"flags": v()}))
    for rung, v in (("none", lambda: None), ("false", lambda: False), ("true", lambda: True), ("tensor", lambda: f64(3)),
                    ("short", lambda: f64(2)), ("dtype", lambda: torch.zeros(3, dtype=torch.float32))):
        done(f"motion_scores_device/scores={rung}", "motion_scores_device", lambda v=v: (dbatch(3)[:2], {"scores": v()}))
    for rung, v in (("none", lambda: None), ("false", lambda: False), ("true", lambda: True), ("tensor", lambda: tensor(3, "centres")),
                    ("short", lambda: tensor(2, "centres")), ("dtype", lambda: tensor(3, "centres", "int64"))):
        done(f"motion_scores_device/terms={rung}", "motion_scores_device", lambda v=v: (dbatch(3)[:2], {"terms": v()}))
    bins = lambda terms=True: (f64(3), torch.zeros(3, dtype=torch.int32) if terms else None, f64(3), dsoff(3), 4)      # noqa: E731
    for rung, v in (("none", lambda: None), ("false", lambda: False), ("true", lambda: True), ("tensor", lambda: torch.zeros((2, 4), dtype=torch.float64)),
                    ("short", lambda: f64(7)), ("dtype", lambda: torch.zeros((2, 4), dtype=torch.float32))):
        done(f"motion_bins_device/acc={rung}", "motion_bins_device", lambda v=v: (bins(), {"acc": v()}))
    for rung, v in (("none", lambda: None), ("false", lambda: False), ("true", lambda: True), ("tensor", lambda: torch.zeros((2, 4), dtype=torch.int64)),
                    ("short", lambda: torch.zeros(7, dtype=torch.int64)), ("dtype", lambda: torch.zeros((2, 4), dtype=torch.int32))):
        done(f"motion_bins_device/bin_terms={rung}", "motion_bins_device", lambda v=v: (bins(), {"bin_terms": v()}))
        done(f"motion_bins_device/no_terms/bin_terms={rung}", "motion_bins_device", lambda v=v: (bins(False), {"bin_terms": v()}))
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)      # noqa: E731
    for rung, v in (("tensor", lambda: i32(2, 3, 3)), ("short", lambda: i32(2, 3, 2)), ("dtype", lambda: torch.zeros((2, 3, 3), dtype=torch.int64))):
        done(f"sweep_centres_device/out={rung}", "sweep_centres_device", lambda v=v: (dbatch(3) + ([4.0, 9.0], [1, 2, 3]), {"out": v()}))
    done("sweep_centres_device/no_settings", "sweep_centres_device", lambda: (dbatch(3) + ([], []), {}))
    done("sweep_centres_device/int32", "sweep_centres_device", lambda: (dbatch(3) + ([4.0], [-2 ** 31 - 1]), {}))
    for rung, v in (("tensor", lambda: i32(2, 8, GH, GW)), ("shape", lambda: i32(2, 8, GH * GW)), ("dtype", lambda: torch.zeros((2, 8, GH, GW), dtype=torch.int64))):
        done(f"flow_map_device/out={rung}", "flow_map_device", lambda v=v: (dbatch(3) + (dsoff(3),), {"out": v()}))

    # ---- device forms: want and out of the six dict- and list-driven scans
    wanted = {
        "activity_map_device": (("active", "centre", "frames"), lambda: dbatch(3) + (dsoff(3),)),
        "scan_dir_device": (("flags", "centres", "rose"), lambda: dbatch(3)),
        "scan_lanes_device": (("flags", "centres", "rose"), lambda: dbatch(3) + (torch.zeros((GH, GW), dtype=torch.uint8),)),
        "scan_blobs_device": (("flags", "centres", "blobs", "largest", "box"), lambda: dbatch(3)),
        "scan_gmc_blobs_device": (("flags", "centres", "blobs", "largest", "box", "info"), lambda: dbatch(3)),
        "persist_device": (("flags", "run", "pos"), lambda: (torch.ones(3, dtype=torch.uint8), dsoff(3))),
    }
    for meth, (names, args) in wanted.items():
        extra = {"work": lambda: torch.zeros(3, dtype=torch.int32)} if meth == "persist_device" else {}
        kw = lambda extra=extra, **k: dict({n: f() for n, f in extra.items()}, **k)      # noqa: E731
        lead = lambda n, meth=meth: 2 if meth == "activity_map_device" else 3      # noqa: E731
        if meth == "scan_blobs_device":
            subsets = [s for r in range(len(names) + 1) for s in itertools.combinations(names, r)]
        else:
            subsets = [(n,) for n in names] + [names]
        for s in subsets:
            done(f"{meth}/want={','.join(s)}", meth, lambda a=args, kw=kw, s=s: (a(), kw(want=s)))
        done(f"{meth}/want=list_reversed", meth, lambda a=args, kw=kw, s=names: (a(), kw(want=list(reversed(s)))))
        done(f"{meth}/want=unknown", meth, lambda a=args, kw=kw, s=names: (a(), kw(want=(s[0], "nothing"))))
        done(f"{meth}/out=full", meth, lambda a=args, kw=kw, s=names, lead=lead: (a(), kw(out={n: tensor(lead(n), n) for n in s})))
        done(f"{meth}/out=partial", meth, lambda a=args, kw=kw, s=names, lead=lead: (a(), kw(out={s[-1]: tensor(lead(s[-1]), s[-1])})))
        done(f"{meth}/out=unwanted", meth, lambda a=args, kw=kw, s=names, lead=lead: (a(), kw(want=s[:1], out={n: tensor(lead(n), n) for n in s})))
        for n in names:
            done(f"{meth}/out={n}:dtype", meth, lambda a=args, kw=kw, n=n, lead=lead: (a(), kw(out={n: tensor(lead(n), n, "float32")})))
            done(f"{meth}/out={n}:shape", meth, lambda a=args, kw=kw, n=n, lead=lead: (a(), kw(out={n: tensor(lead(n) + 1, n)})))

    # ---- device forms: the other refusals
    for meth, other in (("scan_dir_device", "d_allow"), ("scan_blobs_device", "d_keep"), ("scan_gmc_blobs_device", "d_keep")):
        done(f"{meth}/alone:d_stream_off", meth, lambda: (dbatch(3), {"d_stream_off": dsoff(3)}))
        done(f"{meth}/alone:{other}", meth, lambda o=other: (dbatch(3), {o: dkeep(3) if o == "d_keep" else torch.zeros(2, dtype=torch.uint8)}))
    done("scan_blobs_device/keep_size", "scan_blobs_device", lambda: (dbatch(3), {"d_stream_off": dsoff(3), "d_keep": dkeep(1)}))
    done("scan_zones_device/keep_size", "scan_zones_device", lambda: (dbatch(3) + (dsoff(3), dkeep(1)), {}))
    done("scan_zones_device/off_dtype", "scan_zones_device", lambda: (dbatch(3)[:1] + (torch.tensor(OFFS[3], dtype=torch.int32), None, dsoff(3), dkeep(3)), {}))
    done("scan_lanes_device/planes_size", "scan_lanes_device", lambda: (dbatch(3) + (torch.zeros((GH, GW + 1), dtype=torch.uint8),), {}))
    done("scan_lanes_device/no_streams", "scan_lanes_device", lambda: (dbatch(3) + (torch.zeros((GH, GW), dtype=torch.uint8),), {"d_stream_off": dsoff(0)}))
    done("count_centres_device/strided_records", "count_centres_device", lambda: ((torch.zeros(400, dtype=torch.uint8)[::2],) + dbatch(3)[1:], {}))
    done("persist_device/short_work", "persist_device", lambda: ((torch.ones(3, dtype=torch.uint8), dsoff(3)), {"work": torch.zeros(2, dtype=torch.int32)}))
    done("persist_device/box_shape", "persist_device", lambda: ((torch.ones(3, dtype=torch.uint8), dsoff(3)), {
        "d_box": tensor(2, "box"), "work": torch.zeros(3, dtype=torch.int32)}))
    done("merge_streams_device/out_shape", "merge_streams_device", lambda: (
        (None, f64(3), dsoff(3), torch.zeros(64, dtype=torch.uint8)),
        {"seg_cap": 8, "out": (torch.zeros((2, 4, 2), dtype=torch.float64), torch.zeros((2, 40), dtype=torch.uint8), f64(6))}))

    # ---- ScanPipe through __new__
    reports = ("centres", "largest", "vector", "sectors", "", None, 3)
    setters = {"set_blobs": lambda r: ((3,), {"report": r}), "set_gmc": lambda r: ((5, 77), {"report": r}),
               "set_gmc_blobs": lambda r: ((3, 5, 77), {"report": r}), "set_dir": lambda r: ((0x0F,), {"report": r}),
               "set_plane": lambda r: ((np.full((GH, GW), 255, np.uint8),), {"report": r})}
    for meth, fn in setters.items():
        for r in reports:
            one(f"pipe/{meth}/report={r!r}", meth, lambda m, fn=fn, r=r: fn(r), "pipe")
        one(f"pipe/{meth}/defaults", meth, lambda m, fn=fn: (fn(None)[0][:1], {}), "pipe")
    for meth in ("clear_gmc", "clear_gmc_blobs", "clear_dir", "clear_plane"):
        one(f"pipe/{meth}", meth, lambda m: ((), {}), "pipe")
    one("pipe/set_blobs/off", "set_blobs", lambda m: ((0,), {}), "pipe")
    one("pipe/set_dir/names", "set_dir", lambda m: (("E,SE",), {"report": "sectors"}), "pipe")
    one("pipe/set_dir/name_list", "set_dir", lambda m: ((["E", "SE"],), {}), "pipe")
    one("pipe/set_dir/numpy_int", "set_dir", lambda m: ((np.uint8(3),), {}), "pipe")
    one("pipe/set_plane/dtype", "set_plane", lambda m: ((np.zeros((GH, GW), np.int32),), {}), "pipe")
    one("pipe/set_plane/shape", "set_plane", lambda m: ((np.zeros((GW, GH), np.uint8),), {}), "pipe")
    one("pipe/set_plane/strided", "set_plane", lambda m: ((np.zeros((GH, 2 * GW), np.uint8)[:, ::2],), {}), "pipe")
    one("pipe/set_keep/none", "set_keep", lambda m: ((None,), {}), "pipe")
    one("pipe/set_keep/bool", "set_keep", lambda m: ((np.ones((GH, GW), bool),), {}), "pipe")
    one("pipe/set_keep/packed", "set_keep", lambda m: ((np.ones((GH, KW), np.uint64),), {}), "pipe")
    one("pipe/set_keep/bool_shape", "set_keep", lambda m: ((np.ones((GH, GW - 1), bool),), {}), "pipe")
    one("pipe/set_keep/packed_shape", "set_keep", lambda m: ((np.ones((GH, 1), np.uint64),), {}), "pipe")
    for rc in (0, 1):
        one(f"pipe/has_keep/rc={rc}", "has_keep", lambda m: ((), {}), "pipe", {"mtgpu_pipe_has_keep": lambda a, rc=rc: rc})
    for meth in ("blobs", "gmc", "gmc_blobs", "dir", "plane"):
        one(f"pipe/{meth}/off", meth, lambda m: ((), {}), "pipe", {"mtgpu_pipe_" + meth: lambda a: 0})
        for code in (0, 1, 2, 3):
            one(f"pipe/{meth}/code={code}", meth, lambda m: ((), {}), "pipe", {"mtgpu_pipe_" + meth: lambda a, code=code: _answer(a, code)})
    return out


def _answer(args, code):
    """A getter of the library: writes 11, 12, ... through its outputs, then the report code, and says "on"."""
    for i, a in enumerate(args[1:-1]):
        if isinstance(a, _BYREF):
            a._obj.value = 11 + i
    args[-1]._obj.value = code
    return 1


# ---------------------------------------------------------------- signatures
def signatures(mod):
    """Every public function, method and property of the scanner module -> its signature as text."""
    def text(f):
        return str(inspect.signature(f)).replace(mod.__name__ + ".", "")
    out = {}
    for name, v in vars(mod).items():
        if name.startswith("_") or getattr(v, "__module__", None) != mod.__name__:
            continue
        if inspect.isfunction(v):
            out[name] = text(v)
        elif inspect.isclass(v):
            out[name] = text(v)
            for k in dir(v):
                if k.startswith("_"):
                    continue
                a = inspect.getattr_static(v, k)
                if isinstance(a, property):
                    out[f"{name}.{k}"] = "property" + text(a.fget)
                elif isinstance(a, (staticmethod, classmethod)) or inspect.isfunction(a):
                    out[f"{name}.{k}"] = type(a).__name__ + text(getattr(v, k))
    return out


def trace(mod):
    """(signatures, {case id: outcome}) of a scanner module."""
    return signatures(mod), {c[0]: run_case(mod, c) for c in cases()}


def record(path):
    import mvtrim_amd
    sigs, outcomes = trace(load_scanner(path))
    distinct, index = [], {}
    for cid, o in outcomes.items():
        key = json.dumps(o, sort_keys=True)
        if key not in index:
            index[key] = len(distinct)
            distinct.append(key)
        outcomes[cid] = index[key]
    with open(GOLDEN, "w") as f:
        f.write('{"all": %s,\n"signatures": {\n' % json.dumps(sorted(mvtrim_amd.__all__)))
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sigs.items()))
        f.write('},\n"outcomes": [\n' + ",\n".join(distinct) + '],\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {v}" for k, v in outcomes.items()) + "}}\n")
    print(f"{len(outcomes)} cases, {len(distinct)} distinct outcomes, {len(sigs)} signatures -> {GOLDEN}")


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    record(sys.argv[2])
