"""Time one merged video frame (a record, not a gate): ``ops.compose_frame`` on device tensors against the same frame built on
the host with numpy the way the reference's ``save_concatenated_videos`` builds it.

    python tools/frame_timing.py [--height 640 --width 960 --cams 3 --iters 50 --warmup 10]

The frame: the default key set (gt_rgbs, rgbs, depths) of ``--cams`` views.  Device: the median, after a warm-up, of the
intervals between events recorded immediately around the library call (the launch itself is inside, the wrapper's Python is
not), and the GB/s against the bytes the frame moves (12 B per colour pixel and 8 B per depth pixel read, 3 B written).
Host: float32 lists in memory, per frame the depth colouring (log, scale, clip, table lookup -- fp64 after the logarithm),
the concatenations and the cut to 8 bits; the median of ``--host-iters`` runs.  Prints one JSON line.
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


def host_frame(gt, rgb, depth, opacity, table):
    """The reference's arithmetic for one merged frame, in numpy."""
    lo, hi = -np.log(4.0 + 1e-6), -np.log(120 + 1e-6)
    rows = [np.concatenate(gt, axis=1), np.concatenate(rgb, axis=1)]
    coloured = []
    for d, o in zip(depth, opacity):
        v = np.nan_to_num(np.clip((-np.log(d + 1e-6) - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1))
        v *= o
        idx = np.clip((v * 256).astype(np.int64), 0, 255)
        coloured.append(table[idx])
    rows.append(np.concatenate(coloured, axis=1))
    return (255 * np.clip(np.concatenate(rows, axis=0), 0, 1)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--cams", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=5)
    a = ap.parse_args()
    H, W, cams = a.height, a.width, a.cams
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    gt = [torch.rand(H, W, 3, device=dev, generator=g) for _ in range(cams)]
    rgb = [torch.rand(H, W, 3, device=dev, generator=g) for _ in range(cams)]
    depth = [torch.rand(H, W, device=dev, generator=g) * 150 + 1 for _ in range(cams)]
    opacity = [torch.rand(H, W, device=dev, generator=g) for _ in range(cams)]
    tiles = [("colour3", 0, c, gt[c], None) for c in range(cams)] + [("colour3", 1, c, rgb[c], None) for c in range(cams)] \
        + [("depth", 2, c, depth[c], opacity[c]) for c in range(cams)]
    for _ in range(a.warmup):
        frame = ops.compose_frame(tiles, H, W, 3, cams, True)
    torch.cuda.synchronize()
    # events recorded immediately around the library call (the wrapper's Python work stays outside the interval)
    _lib.TIMER = _lib.KernelTimer(["emer_compose_frame"])
    t0 = time.perf_counter()
    for _ in range(a.iters):
        frame = ops.compose_frame(tiles, H, W, 3, cams, True)
    times = _lib.TIMER.elapsed_us()["emer_compose_frame"]
    wall_us = (time.perf_counter() - t0) / a.iters * 1e6
    _lib.TIMER = None
    us = float(np.median(times))
    moved = cams * H * W * (12 + 12 + 8 + 3 * 3)
    lists = [[t.cpu().numpy() for t in lst] for lst in (gt, rgb, depth, opacity)]
    table = ops.turbo_table()
    host = []
    for _ in range(a.host_iters):
        t0 = time.perf_counter()
        ref = host_frame(*lists, table)
        host.append((time.perf_counter() - t0) * 1e3)
    same = float(np.mean(np.all(frame.cpu().numpy() == ref, axis=-1)))
    print(json.dumps({"frame": [3 * H, cams * W, 3], "device_us_median": round(us, 1), "device_us_min": round(float(np.min(times)), 1),
                      "wall_us_per_call": round(wall_us, 1), "bytes_moved": moved, "device_GBps": round(moved / us / 1e3, 1), "host_numpy_ms_median": round(float(np.median(host)), 1),
                      "pixels_equal_to_host": round(same, 6)}))


if __name__ == "__main__":
    main()
