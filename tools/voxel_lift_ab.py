"""Same-session A/B of the voxel-lift kernels (csrc/voxels.hip) against the reference's torch chain on the device
(utils/visualization_tools.py:546-567, :599-612, :634-638): a dense fp32 grid, ``index_put``, ``torch.nonzero`` and a boolean
gather.  One MI355X, one process:

    python tools/voxel_lift_ab.py --out profiles/voxel_lift_ab.json

Shapes: the default box (configs/default_config.yaml:42, expanded as the visualisation does) at the default 0.3 m voxels and at
0.15 m, 640 x 960 rays per image with synthetic end points (about a fifth of them beyond the 80 m cut-off or outside the box).

* ``mark``: one image into the static grid -- the torch chain with its int64 temporaries and ``index_put`` against ``VoxelGrid.mark``.
* ``readout``: ``voxel_coords_to_world_coords(torch.nonzero(grid))`` against ``VoxelGrid.occupied_points`` (both end in one host
  synchronisation: ``nonzero`` has its own), after ten images were marked.
* ``select``: ``points[mean(stack(densities), 0) > 0.5]`` of a 2^18-point chunk, three density arrays, against
  ``ops.mean_threshold_bits`` + ``ops.bits_select_rows``.

Times are per call: medians over ``--reps`` windows between HIP events, torch / kernel windows alternating in one process.  Every
stage also records whether the two sides returned the same tensor.
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
from emernerf_amd.voxels import VoxelGrid, vis_aabb  # noqa: E402

DEV = torch.device("cuda:0")
AABB = [-20.0, -40.0, 0.0, 80.0, 40.0, 20.0]
H, W = 640, 960


def time_us(fns, reps, warmup=2, inner=1):
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


def image(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = H * W
    o = torch.stack([torch.rand(n, device=DEV, generator=g) * 60, torch.rand(n, device=DEV, generator=g) * 4 - 2,
                     torch.rand(n, device=DEV, generator=g) + 1.5], -1)
    d = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0], device=DEV) + 0.6 * torch.randn(n, 3, device=DEV, generator=g), dim=-1)
    t = torch.rand(n, 1, device=DEV, generator=g) * 95 + 1
    return o.reshape(H, W, 3), d.reshape(H, W, 3), t.reshape(H, W, 1)


def torch_mark(grid, o, d, depth, aabb_min, aabb_max, res):
    """:546-567 with datasets/utils.py:85-88 inlined."""
    world = o + d * depth
    world = world[depth.squeeze() < 80]
    voxel_size = (aabb_max - aabb_min) / res
    vc = ((world - aabb_min) / voxel_size).long()
    sel = ((vc[..., 0] >= 0) & (vc[..., 0] < res[0]) & (vc[..., 1] >= 0) & (vc[..., 1] < res[1])
           & (vc[..., 2] >= 0) & (vc[..., 2] < res[2]))
    grid[vc[..., 0][sel], vc[..., 1][sel], vc[..., 2][sel]] = 1


def torch_readout(grid, aabb_min, aabb_max, res):
    return aabb_min + torch.nonzero(grid) * ((aabb_max - aabb_min) / res)


def run(size, reps):
    box = vis_aabb(AABB)
    vg = VoxelGrid(box, size, DEV)
    aabb_min, aabb_max = box[:3].to(DEV), box[3:].to(DEV)
    res = torch.tensor(vg.res, device=DEV)
    dense = torch.zeros(*vg.res, device=DEV)
    images = [image(100 + i) for i in range(10)]
    o, d, t = images[0]
    mark = time_us([lambda: torch_mark(dense, o, d, t, aabb_min, aabb_max, res), lambda: vg.mark(o, d, t, 80.0)], reps, inner=5)
    dense.zero_()
    vg.clear()
    for o_, d_, t_ in images:
        torch_mark(dense, o_, d_, t_, aabb_min, aabb_max, res)
        vg.mark(o_, d_, t_, 80.0)
    a, b = torch_readout(dense, aabb_min, aabb_max, res), vg.occupied_points()
    same = bool(a.shape == b.shape and torch.equal(a, b))
    read = time_us([lambda: torch_readout(dense, aabb_min, aabb_max, res), lambda: vg.occupied_points()], reps)
    out = {"voxel_size": size, "res": list(vg.res), "voxels": vg.n_voxels, "rays_per_image": H * W, "occupied_after_10_images": int(b.shape[0]),
           "dense_grid_bytes": vg.n_voxels * 4, "bit_mask_bytes": vg.bits.numel() * 4, "same_points": same,
           "mark_us": {"torch": mark[0], "hip": mark[1], "speedup_median": mark[0]["median"] / mark[1]["median"]},
           "readout_us": {"torch": read[0], "hip": read[1], "speedup_median": read[0]["median"] / read[1]["median"]}}
    del dense
    return out


def run_select(reps):
    g = torch.Generator(device=DEV).manual_seed(7)
    n = 2 ** 18
    dens = [torch.rand(n, device=DEV, generator=g) for _ in range(3)]
    pts = torch.randn(n, 3, device=DEV, generator=g)
    t_fn = lambda: pts[torch.mean(torch.stack(dens, 0), 0) > 0.5]  # noqa: E731
    h_fn = lambda: ops.bits_select_rows(ops.mean_threshold_bits(dens, 0.5), pts)  # noqa: E731
    a, b = t_fn(), h_fn()
    tm = time_us([t_fn, h_fn], reps)
    return {"points": n, "arrays": 3, "kept": int(b.shape[0]), "same_rows_kept": int(a.shape[0]) == int(b.shape[0]),
            "rows_differing": int((a != b).any(-1).sum()) if a.shape == b.shape else None,
            "select_us": {"torch": tm[0], "hip": tm[1], "speedup_median": tm[0]["median"] / tm[1]["median"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/voxel_lift_ab.json")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voxel_lift_ab: needs the GPU; there is nothing to measure without it")
    res = {"what": "voxel-lift kernels (csrc/voxels.hip) against the reference's torch chain on the device, one MI355X, one process, alternating",
           "device": torch.cuda.get_device_name(0), "grids": [run(s, args.reps) for s in (0.3, 0.15)], "select": run_select(args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
