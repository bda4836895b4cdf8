"""Record tests/golden/ssim_skimage.npz with scikit-image ITSELF (numpy + scikit-image only, no torch: runs under any Python
that has scikit-image).

    python tests/golden/record_ssim_skimage.py

Every case: two fp32 images, a mask, and what skimage.metrics.structural_similarity(x, y, data_range=1.0) returns for them
with the colour axis last -- the scalar, the full S map (``full=True``) and the masked mean ``S[mask].mean()`` of
radiance_fields/video_utils.py:224-233.  scikit-image 0.18 spells the colour axis ``multichannel=True``, 0.19+
``channel_axis=-1``; the algorithm (float64 throughout) is the same.  The inputs are a pure function of ``make_cases()``
(seeded numpy), so tests/test_eval_metrics_cpu.py can regenerate them.
"""
from __future__ import annotations

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

RANDOM_SHAPES = {"rand_7x7x3": (7, 7, 3), "rand_16x24x3": (16, 24, 3), "rand_37x53x3": (37, 53, 3), "rand_48x64x1": (48, 64, 1)}


def make_cases():
    """name -> (x, y, mask): fp32 [H, W, C] images in [0, 1] and a bool [H, W] mask."""
    cases = {}
    for k, (name, shape) in enumerate(RANDOM_SHAPES.items()):
        rng = np.random.default_rng(100 + k)
        x = rng.random(shape).astype(np.float32)
        y = np.clip(x + 0.15 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
        mask = rng.random(shape[:2]) < 0.3
        mask[shape[0] // 2, shape[1] // 2] = True
        cases[name] = (x, y, mask)
    # bright, flat, low noise: uxx - ux^2 cancels -- fp32 moments are off by ~2e-4 per pixel here
    rng = np.random.default_rng(200)
    shape = (64, 96, 3)
    x = (0.9 + 0.002 * rng.standard_normal(shape)).astype(np.float32)
    y = (x + 0.001 * rng.standard_normal(shape)).astype(np.float32)
    cases["bright_flat"] = (x, y, rng.random(shape[:2]) < 0.2)
    # constant regions (zero variance in one or both images), one of them identical in both
    rng = np.random.default_rng(300)
    shape = (32, 40, 3)
    x = rng.random(shape).astype(np.float32)
    y = np.clip(x + 0.1 * rng.standard_normal(shape), 0.0, 1.0).astype(np.float32)
    x[:16, :20] = 0.25
    y[:16, :20] = 0.25
    x[16:, 20:] = 0.7
    y[16:, 20:] = 0.4
    y[:16, 20:] = 1.0
    mask = np.zeros(shape[:2], bool)
    mask[4:28, 8:32] = True
    cases["constant"] = (x, y, mask)
    return cases


def main():
    import skimage
    from skimage.metrics import structural_similarity
    major, minor = (int(v) for v in skimage.__version__.split(".")[:2])
    axis = dict(channel_axis=-1) if (major, minor) >= (0, 19) else dict(multichannel=True)
    out = {"skimage_version": np.array(skimage.__version__)}
    for name, (x, y, mask) in make_cases().items():
        s, S = structural_similarity(x, y, data_range=1.0, full=True, **axis)
        out.update({f"{name}/x": x, f"{name}/y": y, f"{name}/mask": mask, f"{name}/ssim": np.array(s, np.float64),
                    f"{name}/map": S.astype(np.float64), f"{name}/masked_ssim": np.array(S[mask].mean(), np.float64)})
    path = os.path.join(HERE, "ssim_skimage.npz")
    np.savez_compressed(path, **out)
    print(f"ssim_skimage: scikit-image {skimage.__version__}, {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
