"""Time a five-camera merged video frame (a record, not a gate): ``ops.five_view_frame`` -- the reference's picture, the two outer
views shrunk by the cubic-spline zoom -- against ``ops.compose_frame`` on the same 25 tiles, which is what
``five_view_resize=False`` composes (the five views tiled unresized).

    python tools/five_view_timing.py [--sizes 640x960,160x240 --iters 200 --warmup 20 --out profiles/five_view_ab.json]

The frame: five keys (gt_rgbs, rgbs, depths, gt_sky_masks, sky_masks) of five views on device tensors.  Per size, the two
ways alternate in rounds of ``--iters`` calls; a round's time per frame is a host clock around the calls, closed by a device
synchronise (allocation of the frame and the wrapper's Python included: what ``compose_video_frames`` pays per frame), and the
median over the rounds is reported.  The launches alone -- ``emer_zoom_tiles`` on its 10 tiles, ``emer_compose_frame`` on 15 and
on 25 -- are the medians of event intervals recorded immediately around the library calls, in rounds of their own.  For
orientation, where scipy is installed, the host route that the zoom launch replaces for ONE resized colour view: download,
``scipy.ndimage.zoom(img, [h / H, 1, 1])``, upload.  Prints one JSON line and, with ``--out``, writes it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emernerf_amd import _lib, ops  # noqa: E402


def frame_tiles(H, W, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    tiles = []
    for c in range(5):
        tiles += [("colour3", 0, c, torch.rand(H, W, 3, device=dev, generator=g), None),
                  ("colour3", 1, c, torch.rand(H, W, 3, device=dev, generator=g), None),
                  ("depth", 2, c, torch.rand(H, W, device=dev, generator=g) * 150 + 1, torch.rand(H, W, device=dev, generator=g)),
                  ("grey1", 3, c, (torch.rand(H, W, device=dev, generator=g) < 0.4).float(), None),
                  ("one_minus_grey1", 4, c, torch.rand(H, W, device=dev, generator=g), None)]
    return tiles


def per_frame_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure(H, W, iters, warmup, rounds, dev):
    tiles = frame_tiles(H, W, dev)
    ways = {"zoom": lambda: ops.five_view_frame(tiles, H, W, 5, True), "unresized": lambda: ops.compose_frame(tiles, H, W, 5, 5, True)}
    for fn in ways.values():
        for _ in range(warmup):
            fn()
    wall = {k: [] for k in ways}
    for _ in range(rounds):          # alternating: other work shares the machine
        for k, fn in ways.items():
            wall[k].append(per_frame_us(fn, iters))
    _lib.TIMER = _lib.KernelTimer(["emer_zoom_tiles", "emer_compose_frame"])
    for _ in range(iters):
        ways["zoom"]()
    split = _lib.TIMER.elapsed_us()
    _lib.TIMER = _lib.KernelTimer(["emer_compose_frame"])
    for _ in range(iters):
        ways["unresized"]()
    whole = _lib.TIMER.elapsed_us()
    _lib.TIMER = None
    h = ops.five_view_rows(W)
    res = {"size": [H, W], "h": h, "frame": [5 * H, 5 * W, 3], "iters": iters, "rounds": rounds,
           "frame_us": {k: round(float(np.median(v)), 1) for k, v in wall.items()},
           "frame_us_rounds": {k: [round(x, 1) for x in v] for k, v in wall.items()},
           "launch_us_median": {"zoom_tiles_10": round(float(np.median(split["emer_zoom_tiles"])), 1),
                                "compose_frame_15": round(float(np.median(split["emer_compose_frame"])), 1),
                                "compose_frame_25": round(float(np.median(whole["emer_compose_frame"])), 1)}}
    res["zoom_over_unresized"] = round(res["frame_us"]["zoom"] / res["frame_us"]["unresized"], 2)
    # the zoom launch's work, from the shapes: source values it filters (each read by every row block within the warm-up of it)
    # and fp64 operations (csrc/frames.hip: 3 per upward step, 5 in the tail, 2 per downward step, 7 + the weights per output)
    cols = 2 * (3 * W * 3 + 2 * W)            # per frame: 2 views x (2 colour rows + 1 depth row at 3 W, 2 mask rows at W)
    blocks = -(-H // 32)
    steps_up, steps_tail, steps_down, outs = blocks * 36 + H + 2 * blocks, blocks * 37, H + 2 * blocks, h
    flop = cols * (3 * steps_up + 5 * steps_tail + 2 * steps_down + 27 * outs)
    us = res["launch_us_median"]["zoom_tiles_10"]
    res["zoom_launch"] = {"columns": cols, "source_values": cols * H, "fp64_ops": flop, "fp64_Gops_per_s": round(flop / us / 1e3, 1),
                          "source_GBps_if_read_once": round(cols * H * 4 / us / 1e3, 1)}
    try:
        from scipy import ndimage
    except ImportError:
        res["host_route_one_colour_view_ms"] = "not measured (no scipy on this machine)"
        return res
    src = tiles[0][3]
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        z = ndimage.zoom(src.cpu().numpy(), [h / H, 1, 1])
        back = torch.from_numpy(z).to(dev)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    got = ops.zoom_rows(src, h).to(torch.float32)
    res["host_route_one_colour_view_ms"] = round(float(np.median(host)), 2)
    res["max_abs_diff_to_scipy_fp32"] = float((got - back).abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x960,160x240")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "what": "five-camera, five-key merged frame: five_view_frame (zoom) vs compose_frame (unresized)",
           "sizes": [measure(*map(int, s.split("x")), a.iters, a.warmup, a.rounds, dev) for s in a.sizes.split(",")]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
