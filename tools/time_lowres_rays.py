"""Time PixelSource.get_render_rays at a downscale factor against torch's own F.interpolate sequence for the same image
(antialiased bicubic colours + two nearest masks: the resampling part of the reference's get_render_rays, without its rays,
pixel coordinates and feature lookup), same process, alternating, device events around N calls each.

    python tools/time_lowres_rays.py [--out FILE.json] [--height 640 --width 960] [--iters 200]

Both sides include their output allocations and launch overheads: this is the time per image as the eval loop sees it.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--height", type=int, default=640)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    from emernerf_amd.pixel_source import PixelSource
    dev = torch.device("cuda:0")
    n_imgs = 8
    src = PixelSource.synthetic(dev, num_imgs=n_imgs, height=args.height, width=args.width, seed=0, dynamic_ratio=0.1, feature_dim=64)

    def ours(i):
        return src.get_render_rays(i % n_imgs)["pixels"]

    def torch_seq(i, s):
        i %= n_imgs
        rgb = F.interpolate(src.images[i].unsqueeze(0).permute(0, 3, 1, 2), scale_factor=s, mode="bicubic", antialias=True).squeeze(0).permute(1, 2, 0)
        F.interpolate(src.sky_masks[i][None, None], scale_factor=s, mode="nearest")
        F.interpolate(src.dynamic_masks[i][None, None], scale_factor=s, mode="nearest")
        return rgb

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for i in range(args.iters):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters   # us per image

    result = {"device": torch.cuda.get_device_name(0), "height": args.height, "width": args.width, "iters": args.iters, "rounds": args.rounds,
              "unit": "us per image (device events around `iters` calls, allocations and launch overhead included)", "factors": {}}
    for s in (1 / 4, 1 / 16):
        src.update_downscale_factor(s)
        diff = float((ours(3) - torch_seq(3, s)).abs().max())
        for i in range(20):   # warm up both
            ours(i), torch_seq(i, s)
        t_ours, t_torch = [], []
        for _ in range(args.rounds):
            t_ours.append(timed(ours))
            t_torch.append(timed(lambda i: torch_seq(i, s)))
        src.reset_downscale_factor()
        result["factors"][f"1/{round(1 / s)}"] = {
            "get_render_rays_all_keys_us": {"median": statistics.median(t_ours), "min": min(t_ours), "max": max(t_ours)},
            "torch_interpolate_x3_us": {"median": statistics.median(t_torch), "min": min(t_torch), "max": max(t_torch)},
            "max_abs_pixel_difference": diff}
    line = json.dumps(result, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
