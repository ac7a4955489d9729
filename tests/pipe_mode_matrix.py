"""The pipe's scan modes against each other, as a table: what every setter answers in every state, and what it leaves.

A pipe runs one of six scans — plain, blobs, gmc, gmc_blobs, dir, plane — and carries a keep mask or not.  Each case below
is a short list of steps on one of two idle pipes (64 records, 4 frames, 2 buffers on pipe_lanes_inputs.shapes_case()'s
grid; "c" has MT_LAYOUT_CENTRES, "n" has not).  A step either calls a setter — then the return code, mtgpu_last_error()
and, afterwards, all five getters and mtgpu_pipe_has_keep are the answer — or makes the pipe busy ("fill": a batch is
acquired; "flight": an empty batch is submitted) or idle again.  Every case starts from a pipe with every mode and the
mask off and nothing acquired.

    (a) the 20 ordered pairs: X on, Y on, Y off
    (b) X on, X again with other values
    (c) every setter with the report codes -1 .. 5, on both pipes
    (d) every single broken range argument and every pair of them in one call, the off forms included
    (e) the six setters (keep too), on and off form, while a batch is being filled and while one is in flight
    (f) two rungs broken at once: bad report + busy, busy + another mode on, off form + busy
    (g) keep on / off under each mode, each mode on / off under keep
    and the NULL pipe for every setter.

    python tests/pipe_mode_matrix.py --record --commit <id>     writes tests/golden/pipe_mode_matrix.json

records the answers of the library MTGPU_LIBRARY names (default: this tree's) on the GPU.  The fixture is recorded from a
build of the commit BEFORE a change to the setters' code, never from the change itself; tests/test_gpu_pipe_mode_matrix.py
only compares.  Each distinct sentence is stored once (`sentences`); an answer names it by index.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "pipe_mode_matrix.json")

CENTRES, LARGEST, VECTOR, SECTORS = 0, 1, 2, 3           # MT_PIPE_REPORT_*
MODES = ["blobs", "gmc", "gmc_blobs", "dir", "plane"]
SETTER = {"blobs": "mtgpu_pipe_set_blobs", "gmc": "mtgpu_pipe_set_gmc", "gmc_blobs": "mtgpu_pipe_set_gmc_blobs",
          "dir": "mtgpu_pipe_set_dir", "plane": "mtgpu_pipe_set_plane", "keep": "mtgpu_pipe_set_keep"}
# the values the modes' own refusal tests use; "a" / "b" / "k": the two planes and the keep mask of shapes_case()
ON = {"blobs": (3, LARGEST), "gmc": (1, 4, 100, VECTOR), "gmc_blobs": (2, 5, 90, LARGEST), "dir": (1, 0x5B, SECTORS),
      "plane": ("a", SECTORS), "keep": ("k",)}
# the same without a report that needs MT_LAYOUT_CENTRES: accepted by the pipe "n" too
ON_PLAIN = {"blobs": (3, CENTRES), "gmc": (1, 4, 100, CENTRES), "gmc_blobs": (2, 5, 90, CENTRES), "dir": (1, 0x5B, CENTRES),
            "plane": ("a", CENTRES)}
OTHER = {"blobs": (5, CENTRES), "gmc": (1, 7, 50, CENTRES), "gmc_blobs": (4, 9, 30, VECTOR), "dir": (1, 0x11, CENTRES),
         "plane": ("b", CENTRES)}
OFF = {"blobs": (0, 0), "gmc": (0, 0, 0, 0), "gmc_blobs": (0, 0, 0, 0), "dir": (0, 0, 0), "plane": (None, 0), "keep": (None,)}
REPORT_AT = {"blobs": 1, "gmc": 3, "gmc_blobs": 3, "dir": 2, "plane": 1}        # the report's place in the arguments
# (label, argument index, broken value): every range rung of every setter
BREAKS = {"blobs": [("min_blob_neg", 0, -1)],
          "gmc": [("max_shift_neg", 1, -1), ("max_shift_big", 1, 128), ("min_share_neg", 2, -1), ("min_share_big", 2, 257)],
          "gmc_blobs": [("min_blob_neg", 0, -1), ("max_shift_neg", 1, -1), ("max_shift_big", 1, 128), ("min_share_neg", 2, -1),
                        ("min_share_big", 2, 257)],
          "dir": [("allow_neg", 1, -1), ("allow_big", 1, 256)],
          "plane": []}
BAD_REPORT = 7


def call(mode, args):
    return ("set", mode, tuple(args))


def with_arg(args, at, value):
    args = list(args)
    args[at] = value
    return tuple(args)


def cases():
    """[(case id, pipe "c" / "n", [steps])]; a step is ("set", mode, args), ("fill",), ("flight",) or ("idle",)."""
    out = []
    for x, y in itertools.permutations(MODES, 2):                                  # (a)
        out.append((f"a/{x}/{y}", "c", [call(x, ON[x]), call(y, ON[y]), call(y, OFF[y])]))
        out.append((f"a/{x}/{y}/n", "n", [call(x, ON_PLAIN[x]), call(y, ON_PLAIN[y]), call(y, OFF[y])]))
    for x in MODES:                                                                # (b)
        out.append((f"b/{x}", "c", [call(x, ON[x]), call(x, OTHER[x]), call(x, OFF[x]), call(x, OFF[x])]))
    for x in MODES:                                                                # (c)
        for pipe in "cn":
            for r in range(-1, 6):
                out.append((f"c/{x}/{pipe}/{r}", pipe, [call(x, with_arg(ON[x], REPORT_AT[x], r))]))
    for x in MODES:                                                                # (d)
        breaks = BREAKS[x] + [("report", REPORT_AT[x], BAD_REPORT)]
        singles = [[b] for b in breaks]
        pairs = [[p, q] for p, q in itertools.combinations(breaks, 2) if p[1] != q[1]]
        for group in singles + pairs:
            label = "+".join(b[0] for b in group)
            on, off = ON[x], OFF[x]
            for _, at, v in group:
                on = with_arg(on, at, v)
                if not (at == 0 and x != "plane"):                                 # argument 0 is what makes it the off form
                    off = with_arg(off, at, v)
            out.append((f"d/{x}/{label}", "c", [call(x, on)]))
            out.append((f"d/{x}/{label}/off", "c", [call(x, ON[x]), call(x, off)]))
    for x in MODES + ["keep"]:                                                     # (e)
        for busy in ("fill", "flight"):
            out.append((f"e/{x}/{busy}/on", "c", [(busy,), call(x, ON[x]), ("idle",), call(x, ON[x])]))
            out.append((f"e/{x}/{busy}/off", "c", [call(x, ON[x]), (busy,), call(x, OFF[x]), ("idle",), call(x, OFF[x])]))
    for x in MODES:                                                                # (f)
        for busy in ("fill", "flight"):
            out.append((f"f/{x}/bad_report+{busy}", "c", [(busy,), call(x, with_arg(ON[x], REPORT_AT[x], BAD_REPORT)), ("idle",)]))
            out.append((f"f/{x}/needs_centres+{busy}", "n", [(busy,), call(x, ON[x]), ("idle",)]))
            for label, at, v in BREAKS[x]:
                out.append((f"f/{x}/{label}+{busy}", "c", [(busy,), call(x, with_arg(ON[x], at, v)), ("idle",)]))
        for y in MODES:
            if y != x:
                out.append((f"f/{x}/{y}/busy+other", "c", [call(x, ON[x]), ("fill",), call(y, ON[y]), call(y, OFF[y]), ("idle",)]))
                out.append((f"f/{x}/{y}/bad_report+other", "c", [call(x, ON[x]), call(y, with_arg(ON[y], REPORT_AT[y], BAD_REPORT))]))
    for x in MODES:                                                                # (g)
        out.append((f"g/{x}/keep_under_mode", "c", [call(x, ON[x]), call("keep", ON["keep"]), call("keep", OFF["keep"])]))
        out.append((f"g/{x}/mode_under_keep", "c", [call("keep", ON["keep"]), call(x, ON[x]), call(x, OFF[x]),
                                                    call("keep", OFF["keep"])]))
        out.append((f"g/{x}/mode_off_keeps_mask", "n", [call("keep", ON["keep"]), call(x, ON_PLAIN[x]), call("keep", OFF["keep"]),
                                                       call(x, OFF[x])]))
    for x in MODES + ["keep"]:                                                     # the NULL pipe
        out.append((f"null/{x}/on", None, [call(x, ON[x])]))
        out.append((f"null/{x}/off", None, [call(x, OFF[x])]))
    assert len({c[0] for c in out}) == len(out)
    return out


class Rig:
    """The two pipes, the planes and the mask; runs a case and returns its answers."""

    def __init__(self, m, scanner):
        import pipe_lanes_inputs as pl
        from mvtrim_amd import zones
        self.m, self.lib = m, m.load_library()
        p, _, keep, a, b = pl.shapes_case()
        self.params = p
        self.planes = {"a": np.ascontiguousarray(a), "b": np.ascontiguousarray(b)}
        assert not np.array_equal(a, b)
        self.keep = np.ascontiguousarray(zones.pack_keep(keep), dtype=np.uint64)
        self.pipes = {"c": m.ScanPipe(scanner, 64, 4, 2, centres=True), "n": m.ScanPipe(scanner, 64, 4, 2)}
        self.held = None

    def close(self):
        for pipe in self.pipes.values():
            pipe.close()

    def _ptr(self, v):
        if v is None:
            return None
        a = self.keep if v == "k" else self.planes[v]
        return a.ctypes.data_as(C.c_void_p)

    def _set(self, handle, mode, args):
        fn = getattr(self.lib, SETTER[mode])
        if mode in ("plane", "keep"):
            args = (self._ptr(args[0]),) + tuple(args[1:])
        rc = fn(handle, *args)
        return int(rc), ("" if rc == 0 else self.lib.mtgpu_last_error().decode("utf-8", "replace"))

    def state(self, handle):
        """What the five getters and has_keep say; an output a getter leaves alone reads -99."""
        lib, i32, ci = self.lib, C.c_int32, C.c_int
        a, b, c, r = i32(-99), i32(-99), i32(-99), ci(-99)
        st = {"keep": int(lib.mtgpu_pipe_has_keep(handle))}
        st["blobs"] = [int(lib.mtgpu_pipe_blobs(handle, C.byref(a), C.byref(r))), a.value, r.value]
        a, b, c, r = i32(-99), i32(-99), i32(-99), ci(-99)
        st["gmc"] = [int(lib.mtgpu_pipe_gmc(handle, C.byref(a), C.byref(b), C.byref(r))), a.value, b.value, r.value]
        a, b, c, r = i32(-99), i32(-99), i32(-99), ci(-99)
        st["gmc_blobs"] = [int(lib.mtgpu_pipe_gmc_blobs(handle, C.byref(a), C.byref(b), C.byref(c), C.byref(r))), a.value, b.value,
                           c.value, r.value]
        a, r = i32(-99), ci(-99)
        st["dir"] = [int(lib.mtgpu_pipe_dir(handle, C.byref(a), C.byref(r))), a.value, r.value]
        r = ci(-99)
        got = np.full_like(self.planes["a"], 0xA5)
        rc = int(lib.mtgpu_pipe_plane(handle, got.ctypes.data_as(C.c_void_p), C.byref(r)))
        which = [k for k, v in self.planes.items() if np.array_equal(got, v)]
        st["plane"] = [rc, which[0] if which else ("untouched" if (got == 0xA5).all() else "other"), r.value]
        return st

    def _busy(self, handle, how):
        assert self.held is None
        b = C.c_void_p()
        assert self.lib.mtgpu_pipe_acquire(handle, C.byref(b)) == 0
        if how == "flight":
            assert self.lib.mtgpu_pipe_submit(handle, b) == 0                      # an empty batch: an event, no kernel
        self.held = (how, b)

    def _idle(self, handle):
        if self.held is None:
            return
        how, b = self.held
        if how == "flight":
            b = C.c_void_p()
            assert self.lib.mtgpu_pipe_collect(handle, C.byref(b), None, None, None, None) == 0
        assert self.lib.mtgpu_pipe_release(handle, b) == 0
        self.held = None

    def reset(self, handle):
        self._idle(handle)
        for x in MODES + ["keep"]:
            assert self._set(handle, x, OFF[x]) == (0, ""), x
        st = self.state(handle)
        assert st["keep"] == 0 and all(st[x][0] == 0 for x in MODES), st

    def run(self, case):
        _, which, steps = case
        handle = None if which is None else self.pipes[which]._pipe
        if handle is not None:
            self.reset(handle)
        got = []
        for step in steps:
            if step[0] == "set":
                rc, text = self._set(handle, step[1], step[2])
                got.append({"rc": rc, "error": text, "state": self.state(handle)})
            elif step[0] == "idle":
                self._idle(handle)
            else:
                self._busy(handle, step[0])
        if handle is not None:
            self.reset(handle)
        return got


def answers(m, scanner):
    """{case id: [answer per setter call]} of the loaded library."""
    rig = Rig(m, scanner)
    try:
        return {case[0]: rig.run(case) for case in cases()}
    finally:
        rig.close()


def pack(ans):
    """answers -> (sentences, states, {case: [[rc, index of the sentence, index of the state] per setter call]})."""
    sentences = sorted({a["error"] for steps in ans.values() for a in steps})
    states = sorted({json.dumps(a["state"], sort_keys=True) for steps in ans.values() for a in steps})
    at, st = {s: i for i, s in enumerate(sentences)}, {s: i for i, s in enumerate(states)}
    return sentences, [json.loads(s) for s in states], \
        {k: [[a["rc"], at[a["error"]], st[json.dumps(a["state"], sort_keys=True)]] for a in steps] for k, steps in ans.items()}


def unpack(doc):
    return {k: [{"rc": rc, "error": doc["sentences"][e], "state": doc["states"][s]} for rc, e, s in steps] for k, steps in doc["answers"].items()}


def write_fixture(head, sentences, states, packed):
    """One line per sentence, per state and per case: the file stays small enough to read and to diff."""
    def lines(rows):
        return "[\n" + ",\n".join(json.dumps(r, sort_keys=True, separators=(",", ":")) for r in rows) + "\n]"
    with open(FIXTURE, "w") as f:
        f.write("{\n" + "".join('"%s": %s,\n' % (k, json.dumps(v)) for k, v in sorted(head.items())))
        f.write('"sentences": ' + lines(sentences) + ',\n"states": ' + lines(states) + ',\n"answers": {\n')
        f.write(",\n".join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in sorted(packed.items())))
        f.write("\n}\n}\n")


def recorded():
    """The fixture's answers, sentences in place."""
    with open(FIXTURE) as f:
        return unpack(json.load(f))


def excludes_every_other(x, ans=None):
    """What made the order of mtgpu_pipe_submit's tests matter is gone if this holds: while the pipe runs x every other
    mode's on form is refused and leaves x as it was (cases a), x takes new values of its own (case b), and no recorded
    answer anywhere leaves two modes on."""
    ans = ans or recorded()
    for steps in ans.values():
        for a in steps:
            if sum(a["state"][y][0] == 1 for y in MODES) > 1:
                return False
    for y in MODES:
        if y != x:
            on_x, on_y, _ = ans[f"a/{x}/{y}"]
            if on_x["rc"] != 0 or on_x["state"][x][0] != 1 or on_y["rc"] == 0 or on_y["state"] != on_x["state"]:
                return False
    first, again = ans[f"b/{x}"][:2]
    return first["rc"] == again["rc"] == 0 and first["state"][x] != again["state"][x] and again["state"][x][0] == 1


def record(commit):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import mvtrim_amd as m
    import pipe_lanes_inputs as pl
    with m.MotionScanner(pl.shapes_case()[0], device=0) as s:
        sentences, states, packed = pack(answers(m, s))
    write_fixture({"recorded_from": commit, "library": m.load_library().mtgpu_version().decode(),
                   "how": "python tests/pipe_mode_matrix.py --record --commit <id> on the GPU, with MTGPU_LIBRARY naming libmtgpu.so built from that commit"},
                  sentences, states, packed)
    print("recorded", sum(len(v) for v in packed.values()), "answers of", len(packed), "cases,", len(sentences), "sentences, from", commit)


if __name__ == "__main__":
    if "--record" not in sys.argv or "--commit" not in sys.argv:
        raise SystemExit(__doc__)
    sys.path.insert(0, HERE)
    record(sys.argv[sys.argv.index("--commit") + 1])
