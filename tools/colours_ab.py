"""Same-session A/B of the evaluation-colour launches (csrc/colours.hip) against the equivalent torch chain, and the eval loop's
throughput with ``visualize`` off and on.  One MI355X, one process:

    python tools/colours_ab.py --out profiles/colours_ab.json

* ``projection``: one scaled projection of a 640 x 960 image, ``ops.feature_colours`` against ``clamp((feat @ M - lo) / (hi -
  lo), 0, 1) * s``, at E = 64 and E = 768; the achieved share of the 8 TB/s HBM peak from the bytes the kernel has to move
  (N E 4 read, N 4 scale, N 12 written).  A 640 x 960 x 768 image is 1.9 GB: it cannot stay in the 256 MiB Infinity Cache
  between replays; the E = 64 image (157 MB) can, so its figure is an upper bound on what a cold image sees.
* ``image``: every list of a PE-branch image at E = 64 -- six projections and two blends, two launches -- against the torch
  chains of the reference's loop.
* ``loop``: ``render_pixels`` on the feature model over a synthetic source, ``visualize`` off / on alternating, the loop's own
  ``render_rays_per_s``.

Times are per call: medians over ``--reps`` windows of ten calls between HIP events, torch / kernel windows alternating in one
process.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emernerf_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK = 8.0e12


def time_us(fns, reps, warmup=3, inner=10):
    """Median microseconds per call of each callable: ``inner`` calls back to back between two events (the host's work for a call
    hides behind the device's for the call before), the callables alternating window by window."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / inner)
    return [{"median": statistics.median(t), "min": min(t), "max": max(t)} for t in times]


def torch_colours(feat, mat, lo, hi, scale=None):
    x = torch.clamp((feat @ mat - lo) / (hi - lo), 0, 1)
    return x if scale is None else x * scale


def torch_blend(a, o, b):
    return torch.clamp(a * o + b * (1 - o), 0, 1)


def case(N, E, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    feat = torch.randn(N, E, device=DEV, generator=g) * 0.5 + 0.2
    mat = torch.randn(E, 3, device=DEV, generator=g) / E ** 0.5
    p = feat[:4096] @ mat
    return feat, mat, p.quantile(0.2, dim=0), p.quantile(0.8, dim=0), torch.rand(N, 1, device=DEV, generator=g)


def projection(N, E, reps):
    feat, mat, lo, hi, s = case(N, E, E)
    got, want = ops.feature_colours(feat, mat, lo, hi, s), torch_colours(feat, mat, lo, hi, s)
    t_torch, t_hip = time_us([lambda: torch_colours(feat, mat, lo, hi, s), lambda: ops.feature_colours(feat, mat, lo, hi, s)], reps)
    nbytes = N * (E * 4 + 4 + 12)
    return {"rows": N, "E": E, "torch_us": t_torch, "hip_us": t_hip, "speedup_median": t_torch["median"] / t_hip["median"],
            "bytes": nbytes, "hip_GBps": nbytes / t_hip["median"] / 1e3, "hip_fraction_of_8TBps": nbytes / (t_hip["median"] * 1e-6) / HBM_PEAK,
            "max_abs_diff_vs_torch": float((got - want).abs().max())}


def image(N, E, reps):
    names = ("dino_feat", "features", "dino_pe_free", "dino_pe", "static_dino", "dynamic_dino")
    f = {n: case(N, E, 10 + i) for i, n in enumerate(names)}
    g = torch.Generator(device=DEV).manual_seed(99)
    opa, dyn_opa = torch.rand(N, 1, device=DEV, generator=g), torch.rand(N, 1, device=DEV, generator=g)
    dyn_rgb, sta_rgb = torch.rand(N, 3, device=DEV, generator=g), torch.rand(N, 3, device=DEV, generator=g)
    scales = {"dino_pe_free": opa, "dynamic_dino": dyn_opa}

    def hip():
        cols = ops.feature_colours_multi([(f[n][0], *f[n][1:4], scales.get(n)) for n in names])
        return cols + ops.blend_over_multi([(dyn_rgb, dyn_opa, cols[4]), (cols[5], dyn_opa, sta_rgb)])

    def chain():
        cols = [torch_colours(f[n][0], *f[n][1:4], scales.get(n)) for n in names]
        return cols + [torch_blend(dyn_rgb, dyn_opa, cols[4]), torch_blend(cols[5], dyn_opa, sta_rgb)]
    diff = max(float((a - b).abs().max()) for a, b in zip(hip(), chain()))
    t_torch, t_hip = time_us([chain, hip], reps)
    return {"rows": N, "E": E, "lists": 8, "hip_launches": 2, "torch_us": t_torch, "hip_us": t_hip,
            "speedup_median": t_torch["median"] / t_hip["median"], "max_abs_diff_vs_torch": diff}


def loop(rounds):
    from emernerf_amd.pixel_source import PixelSource
    from emernerf_amd.trainer import Trainer, render_config
    from emernerf_amd.video_utils import render_pixels
    tr = Trainer(kind="feature", device=DEV, table_init=0.2, seed=1)
    src = PixelSource.synthetic(DEV, num_imgs=6, height=160, width=240, num_cams=3, seed=4, dynamic_ratio=0.1, feature_dim=64)
    cfg = render_config()
    kw = dict(proposal_networks=tr.props, compute_metrics=True)
    render_pixels(cfg, tr.model, tr.estimator, src, **kw)           # warm-up
    first = render_pixels(cfg, tr.model, tr.estimator, src, visualize=True, **kw)
    res = {"images": len(src), "hw": [160, 240], "off": [], "on": [],
           "new_lists": sorted(k for k in first if "dino" in k and isinstance(first[k], list))}
    for _ in range(rounds):
        res["off"].append(render_pixels(cfg, tr.model, tr.estimator, src, **kw)["render_rays_per_s"])
        res["on"].append(render_pixels(cfg, tr.model, tr.estimator, src, visualize=True, feature_pca=first.get("feature_pca"), **kw)["render_rays_per_s"])
    res["off_median"], res["on_median"] = statistics.median(res["off"]), statistics.median(res["on"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    N = 640 * 960
    with torch.no_grad():
        out = {"what": "evaluation-colour launches (csrc/colours.hip) against the equivalent torch chain, one MI355X, one process, alternating",
               "device": torch.cuda.get_device_name(0),
               "projection": [projection(N, 64, a.reps), projection(N, 768, a.reps)],
               "image": image(N, 64, a.reps),
               "loop": loop(a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
