"""Time one order-statistics call (a record, not a gate) against torch's sort-based evaluation of the same call on the same card.

    python tools/select_timing.py box    [--points 8000000 --iters 30 --warmup 5]
    python tools/select_timing.py depth  [--height 640 --width 960 --iters 100 --warmup 10]

``box``: ``ops.quantile(pts, [0.02, 0.98], dim=0)`` of [points, 3] lidar points -- the scene box of a 200-scan log after the factor-4
downsample -- against ``torch.sort(pts, dim=0)`` followed by the same two reads and lerps (``torch.quantile`` itself refuses more
than 16 777 216 elements).  ``depth``: ``ops.weighted_percentile(depth, opacity, [0.5, 99.5])`` of one image against the reference's
steps in torch (sort, gather of the weights, cumsum, searchsorted and the interpolation).  Each runs in a process of its own.  The
interval lies between events recorded immediately around the library call (its clear, passes and final launch are inside, the
wrapper's Python is not); the wall time per call of the wrapper is printed next to it, and the GB/s against ONE read of the keys
(and weights).  Prints one JSON line.
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


def timed(fn, iters, warmup):
    """(median us, min us) between device events around ``fn``."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return float(np.median(t)), float(np.min(t))


def library(fn, iters, warmup):
    """(median us, min us) of the emer_select calls inside ``fn``, (wall us per call of ``fn``)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    _lib.TIMER = _lib.KernelTimer(["emer_select"])
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    times = _lib.TIMER.elapsed_us()["emer_select"]
    wall = (time.perf_counter() - t0) / iters * 1e6
    _lib.TIMER = None
    per_call = np.asarray(times).reshape(iters, -1).sum(1)
    return float(np.median(per_call)), float(np.min(per_call)), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=("box", "depth"))
    ap.add_argument("--points", type=int, default=8_000_000)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if a.which == "box":
        n = a.points
        pts = torch.randn(n, 3, device=dev, generator=g) * torch.tensor([40.0, 40.0, 5.0], device=dev)
        qs = [0.02, 0.98]

        def mine():
            return ops.quantile(pts, qs, dim=0)

        def by_sort():
            s = torch.sort(pts, dim=0)[0]
            out = []
            for q in qs:
                rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(n - 1, dtype=torch.float32)
                lo, hi = int(torch.floor(rank)), int(torch.ceil(rank))
                out.append(torch.lerp(s[lo], s[hi], float(rank - lo)))
            return torch.stack(out)

        bytes_once = 12 * n
        err = float((mine() - by_sort()).abs().max())
    else:
        H, W = a.height, a.width
        depth = torch.exp(torch.rand(H, W, device=dev, generator=g) * 6.4 - 0.7)
        opacity = torch.clamp(torch.rand(H, W, device=dev, generator=g) * 1.6 - 0.3, 0, 1)
        ps = [0.5, 99.5]

        def mine():
            return ops.weighted_percentile(depth, opacity, ps)

        def by_sort():
            x, idx = torch.sort(depth.reshape(-1))
            acc = torch.cumsum(opacity.reshape(-1)[idx].double(), 0)
            t = torch.tensor(ps, dtype=torch.float64, device=dev) * (acc[-1] / 100)
            k = torch.searchsorted(acc, t, right=True).clamp(1, acc.numel() - 1)
            frac = (t - acc[k - 1]) / (acc[k] - acc[k - 1])
            return x[k - 1].double() + frac * (x[k] - x[k - 1]).double()

        bytes_once = 8 * H * W
        n = H * W
        err = float((mine() - by_sort()).abs().max())
    med, low, wall = library(mine, a.iters, a.warmup)
    s_med, s_low = timed(by_sort, a.iters, a.warmup)
    print(json.dumps({"call": a.which, "rows": n, "select_us_median": round(med, 1), "select_us_min": round(low, 1),
                      "select_wall_us_per_call": round(wall, 1), "bytes_read_once": bytes_once, "select_GBps_of_one_read": round(bytes_once / med / 1e3, 1),
                      "torch_sort_us_median": round(s_med, 1), "torch_sort_us_min": round(s_low, 1), "max_abs_difference": err}))


if __name__ == "__main__":
    main()
