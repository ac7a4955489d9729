#!/usr/bin/env python3
"""What the scan's early exit costs and saves, by where a frame's proof falls (docs/rounds/r33_scan_early_exit.md).

16 384 frames of 1080p dense8x8 (32 640 40-byte records each, four per cell in raster order: 21.4 GB), one generated
frame tiled on the device.  Variants of that frame:
  still        no record moves: never decided, read to the end
  row R        cells (10, R) and (11, R) move: decided in the streaming step that holds row R (first analysed row 3,
               then a quarter, half and three quarters of the way down)
  pan          every record moves: decided within the first step
  checker      the cells with x + y even move: half the cells vote, none has an active 4-neighbour, never decided
Each variant is scanned by a context with the exit on and by one created under MTGPU_EARLY_EXIT=0, alternating, ROUNDS
rounds of STEPS launches; scan-kernel time from the library's profile events.  Flags of the two contexts must agree.
Prints one JSON line per variant."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GW, GH, FRAMES = 120, 68, 16384
ROUNDS, STEPS = 3, 20


def frame(kind):
    import mvtrim_amd as m
    cells = np.arange(GW * GH).repeat(4)
    x, y = cells % GW, cells // GW
    f = np.zeros(len(cells), dtype=m.MV_DTYPE)
    f["dst_x"], f["dst_y"] = x * 16 + 4, y * 16 + 4
    f["src_x"], f["src_y"] = f["dst_x"], f["dst_y"]
    if kind == "pan":
        moving = np.ones(len(cells), dtype=bool)
    elif kind == "checker":
        moving = (x + y) % 2 == 0
    elif kind.startswith("row"):
        moving = (y == int(kind[3:])) & ((x == 10) | (x == 11))
    else:
        moving = np.zeros(len(cells), dtype=bool)
    f["src_x"][moving] -= 7
    return f


def main():
    import torch
    import mvtrim_amd as m
    params = m.ScanParams.from_config(1920, 1080, **m.config.CODE_DEFAULTS)
    os.environ.pop("MTGPU_EARLY_EXIT", None)
    on = m.MotionScanner(params, device=0)
    os.environ["MTGPU_EARLY_EXIT"] = "0"
    off = m.MotionScanner(params, device=0)
    os.environ.pop("MTGPU_EARLY_EXIT")
    from mvtrim_amd import early_exit
    assert early_exit.plan(on)["early_exit"] == 1 and early_exit.plan(off)["early_exit"] == 0
    n = GW * GH * 4
    arena = torch.empty(FRAMES * n * 40, dtype=torch.uint8, device="cuda")
    d_off = torch.arange(FRAMES + 1, dtype=torch.int64, device="cuda") * n
    flags = {"on": torch.empty(FRAMES, dtype=torch.uint8, device="cuda"), "off": torch.empty(FRAMES, dtype=torch.uint8, device="cuda")}
    kinds = sys.argv[1:] or ["still", "row3", "row18", "row34", "row49", "pan", "checker"]
    for kind in kinds:
        tile = torch.from_numpy(frame(kind).view(np.uint8).copy()).cuda()
        arena.view(FRAMES, n * 40)[:] = tile
        ms = {"on": [], "off": []}
        for rnd in range(ROUNDS + 1):                    # round 0 warms up
            for name, s in (("on", on), ("off", off)):
                s.profile(True)
                for _ in range(STEPS):
                    s.check_frames_device(arena, d_off, None, flags[name])
                pr = s.profile_read()
                s.profile(False)
                torch.cuda.synchronize()
                if rnd:
                    ms[name].append(pr["scan_ms"])
        assert torch.equal(flags["on"], flags["off"]), kind
        a, b = float(np.median(ms["on"])), float(np.median(ms["off"]))
        print(json.dumps({"variant": kind, "flag": int(flags["on"][0]), "scan_ms_on": [round(v, 4) for v in ms["on"]],
                          "scan_ms_off": [round(v, 4) for v in ms["off"]], "on_over_off": round(a / b, 4)}), flush=True)


if __name__ == "__main__":
    main()
