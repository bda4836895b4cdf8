"""SSIM restated in float64 numpy, exactly as skimage.metrics.structural_similarity(x, y, data_range=1.0, channel_axis=-1)
computes it with its defaults (scikit-image 0.18-0.20): 7 x 7 uniform window with scipy's 'reflect' borders (numpy's
'symmetric' padding), sample covariance (49 / 48), K1 = 0.01, K2 = 0.03; the scalar is the mean of the S map cropped by 3
pixels, per channel, averaged over channels; ``full=True`` returns the uncropped map as well.

numpy only: the scikit-image recorder (tests/golden/record_ssim_skimage.py) and the tests import it; checked against
scikit-image itself through tests/golden/ssim_skimage.npz (tests/test_eval_metrics_cpu.py)."""
from __future__ import annotations

import numpy as np

WIN = 7
PAD = (WIN - 1) // 2


def _box_mean(a: np.ndarray) -> np.ndarray:
    """7 x 7 mean of a 2-D array, reflect borders (scipy.ndimage.uniform_filter(a, 7, mode='reflect'))."""
    p = np.pad(a, PAD, mode="symmetric")
    H, W = a.shape
    rows = sum(p[i:i + H, :] for i in range(WIN))          # separable 7-tap sums (no running sums: no cancellation)
    return sum(rows[:, j:j + W] for j in range(WIN)) / (WIN * WIN)


def ssim_map_2d(x: np.ndarray, y: np.ndarray, data_range: float = 1.0) -> np.ndarray:
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if min(x.shape) < WIN:
        raise ValueError("image smaller than the 7 x 7 window")
    ux, uy = _box_mean(x), _box_mean(y)
    uxx, uyy, uxy = _box_mean(x * x), _box_mean(y * y), _box_mean(x * y)
    cov_norm = WIN * WIN / (WIN * WIN - 1.0)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    A1, A2 = 2 * ux * uy + C1, 2 * vxy + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim(x: np.ndarray, y: np.ndarray, full: bool = False):
    """[H, W, C] (or [H, W]) images -> the scalar (and the [H, W, C] / [H, W] S map with ``full``)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    two_d = x.ndim == 2
    if two_d:
        x, y = x[..., None], y[..., None]
    maps = [ssim_map_2d(x[..., c], y[..., c]) for c in range(x.shape[-1])]
    mssim = float(np.mean([m[PAD:-PAD, PAD:-PAD].mean() for m in maps]))
    if not full:
        return mssim
    S = np.stack(maps, axis=-1)
    return mssim, (S[..., 0] if two_d else S)


def masked_ssim(x: np.ndarray, y: np.ndarray, mask: np.ndarray) -> float:
    """structural_similarity(..., full=True)[1][mask.astype(bool)].mean() (radiance_fields/video_utils.py:224-233)."""
    _, S = ssim(x, y, full=True)
    return float(S[np.asarray(mask).reshape(S.shape[:2]).astype(bool)].mean())
