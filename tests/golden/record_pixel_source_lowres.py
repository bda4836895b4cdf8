"""Record the low-resolution pixel-source fixture by running the REFERENCE's own Python on CPU (build container only):

    python tests/golden/record_pixel_source_lowres.py

pixel_source_lowres.npz: datasets/base/pixel_source.py's ScenePixelSource, UNMODIFIED (loaded by file path as
record_eval_metrics.py loads it), with sky masks, dynamic masks, features (5 x 7 x 4), 3 cameras and timestamps:

* ``get_render_rays`` of images 0..2 after ``update_downscale_factor(s)`` for three cases

      A  37 x 53   s = 1/4    9 x 13   H s is not an integer (the mapping scale is 1 / s, not H / h)
      B  37 x 53   s = 1/3   12 x 17   s is not a power of two: the scaled intrinsics and the nearest index round
      C  100 x 72  s = 1/16   6 x 4    the filter window is wider than half the image: every output renormalises at a border

  on structured images (uniform noise averages to 0.45 - 0.55 and hides a wrong filter): image 0 a ramp plus a checkerboard,
  image 1 isolated unit impulses at the four corners, the centre and one pixel off each border (their responses are the
  filter weights themselves), image 2 random.  A and B share their source tensors.
* ``update_pixel_error_maps`` on seeded rgbs / gt_rgbs / dynamic_opacities lists at the buffer shape of case A ([3, 9, 13]).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"A": dict(hw=(37, 53), factor=1 / 4, out_hw=(9, 13)),
         "B": dict(hw=(37, 53), factor=1 / 3, out_hw=(12, 17)),
         "C": dict(hw=(100, 72), factor=1 / 16, out_hw=(6, 4))}
FEAT_HW, FEAT_DIM, N_IMGS, NUM_CAMS = (5, 7), 4, 3, 3
ERROR_SEED, BUFFER_DOWNSCALE = 1700, 4


def impulse_positions(H: int, W: int):
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (1, W // 2), (H - 2, W // 2), (H // 2, 1), (H // 2, W - 2)]


def source_tensors(hw, seed: int = 1600):
    """Seeded dataset tensors of one source size."""
    H, W = hw
    g = torch.Generator().manual_seed(seed + H)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ramp = torch.stack([xx / (W - 1), yy / (H - 1), (xx + yy) / (H + W - 2)], dim=-1)
    checker = ((torch.floor(xx / 3) + torch.floor(yy / 2)) % 2)[..., None] * 0.25
    images = torch.zeros(N_IMGS, H, W, 3)
    images[0] = (0.75 * ramp + checker).clamp(0, 1)
    for y, x in impulse_positions(H, W):
        images[1, y, x] = 1.0
    images[2] = torch.rand(H, W, 3, generator=g)
    sky = (torch.rand(N_IMGS, H, W, generator=g) < 0.2).float()
    dyn = (torch.rand(N_IMGS, H, W, generator=g) < 0.3).float()
    feats = torch.rand(N_IMGS, FEAT_HW[0], FEAT_HW[1], FEAT_DIM, generator=g)
    c2w = torch.eye(4).repeat(N_IMGS, 1, 1)
    for i in range(N_IMGS):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        c2w[i, :3, :3] = q
        c2w[i, :3, 3] = torch.randn(3, generator=g) * 10
    K = torch.tensor([[0.9 * W, 0.0, W / 2 + 0.3], [0.0, 0.8 * W, H / 2 - 0.2], [0.0, 0.0, 1.0]]).repeat(N_IMGS, 1, 1)
    K[:, 0, 0] += torch.rand(N_IMGS, generator=g)
    ts = torch.tensor([0.0, 0.5, 1.0])
    cams = torch.arange(N_IMGS) % NUM_CAMS
    return dict(images=images, sky_masks=sky, dynamic_masks=dyn, features=feats, cam_to_worlds=c2w, intrinsics=K,
                normalized_timestamps=ts, cam_ids=cams)


def error_lists(seed: int = ERROR_SEED):
    """Seeded render results at the buffer shape of case A."""
    H, W = CASES["A"]["hw"]
    hb, wb = H // BUFFER_DOWNSCALE, W // BUFFER_DOWNSCALE
    g = torch.Generator().manual_seed(seed)
    rgbs = torch.rand(N_IMGS, hb, wb, 3, generator=g)
    gt = torch.rand(N_IMGS, hb, wb, 3, generator=g)
    opa = torch.rand(N_IMGS, hb, wb, generator=g) ** 4     # about 44 % above the 0.1 threshold
    return rgbs, gt, opa


def reference_source(t, hw, buffer_ratio: float = 0.0):
    import importlib.util
    import types
    from oracle import ref_shims
    ref_shims.install()
    fe = types.ModuleType("third_party.feature_extractor")
    fe.delete_features = fe.extract_and_save_features = lambda *a, **k: None
    sys.modules["third_party.feature_extractor"] = fe
    spec = importlib.util.spec_from_file_location("ref_pixel_source", os.path.join(ref_shims.REFERENCE_ROOT, "datasets", "base", "pixel_source.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Source(mod.ScenePixelSource):   # the abstract hooks read files; the tensors are set directly instead
        def create_all_filelist(self):
            pass

        def load_calibrations(self):
            pass

    H, W = hw
    src = Source.__new__(Source)
    src.device = torch.device("cpu")
    src._downscale_factor = src._old_downscale_factor = 1.0
    src.images, src.sky_masks, src.dynamic_masks, src.features = t["images"], t["sky_masks"], t["dynamic_masks"], t["features"]
    src.featmap_downscale_factor = (t["features"].shape[1] / H, t["features"].shape[2] / W)   # :318-321
    src.cam_to_worlds, src.intrinsics = t["cam_to_worlds"], t["intrinsics"]
    src._normalized_timestamps = t["normalized_timestamps"]
    src.cam_ids = t["cam_ids"]
    src.pixel_error_buffered = False
    src.pixel_error_maps = None
    src.data_cfg = ref_shims.ns(load_size=[H, W], num_cams=NUM_CAMS, sampler=dict(buffer_ratio=buffer_ratio, buffer_downscale=BUFFER_DOWNSCALE))
    return src


def run():
    out = {}
    sources = {}
    for name, case in CASES.items():
        hw = case["hw"]
        tag = f"{hw[0]}x{hw[1]}"
        if tag not in sources:
            sources[tag] = source_tensors(hw)
            for k, v in sources[tag].items():
                out[f"src{tag}/{k}"] = v.numpy()
        src = reference_source(sources[tag], hw)
        out[f"{name}/source"] = np.array(tag)
        out[f"{name}/factor"] = np.array(case["factor"], dtype=np.float64)
        src.update_downscale_factor(case["factor"])
        for i in range(N_IMGS):
            rr = src.get_render_rays(i)
            assert tuple(rr["pixels"].shape[:2]) == case["out_hw"], (name, rr["pixels"].shape)
            if i == 0:
                out[f"{name}/keys"] = np.array(sorted(rr))
            for k, v in rr.items():
                out[f"{name}/img{i}/{k}"] = v.numpy()
        src.reset_downscale_factor()
        assert src.downscale_factor == 1.0
    # the error buffer of case A's source
    rgbs, gt, opa = error_lists()
    src = reference_source(sources["37x53"], CASES["A"]["hw"], buffer_ratio=0.5)
    src.build_pixel_error_buffer()
    src.update_pixel_error_maps({"rgbs": [a.numpy() for a in rgbs], "gt_rgbs": [a.numpy() for a in gt],
                                 "dynamic_opacities": [a.numpy() for a in opa]})
    out["error/rgbs"], out["error/gt_rgbs"], out["error/dynamic_opacities"] = rgbs.numpy(), gt.numpy(), opa.numpy()
    out["error/maps"] = src.pixel_error_maps.numpy()
    return out


def main():
    out = run()
    path = os.path.join(HERE, "pixel_source_lowres.npz")
    np.savez_compressed(path, **out)
    print(f"pixel_source_lowres: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
