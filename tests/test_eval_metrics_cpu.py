"""CPU tests of the evaluation-metric fixtures: the float64 SSIM restatement (tests/_ssim_ref.py) against scikit-image's own
recording, and the recorders' inputs regenerated from their seeds."""
import os

import numpy as np
import pytest

from tests import _ssim_ref as R
from tests.golden import record_ssim_skimage as RS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _cases(z):
    return sorted({k.split("/")[0] for k in z.files if "/" in k})


def test_ssim_restatement_matches_skimage_recording():
    """Scalar and masked mean to 1e-12.  The S map to 1e-11: scipy's uniform_filter keeps running sums, whose rounding on the
    bright flat case reaches ~3e-12; the restatement adds the 7 taps directly."""
    z = np.load(os.path.join(GOLDEN, "ssim_skimage.npz"))
    assert str(z["skimage_version"]).startswith("0.")
    names = _cases(z)
    assert {"bright_flat", "constant", "rand_7x7x3", "rand_16x24x3", "rand_37x53x3", "rand_48x64x1"} <= set(names)
    for n in names:
        x, y, mask = z[n + "/x"], z[n + "/y"], z[n + "/mask"]
        s, S = R.ssim(x, y, full=True)
        assert abs(s - float(z[n + "/ssim"])) <= 1e-12, n
        np.testing.assert_allclose(S, z[n + "/map"], rtol=0, atol=1e-11, err_msg=n)
        assert abs(R.masked_ssim(x, y, mask) - float(z[n + "/masked_ssim"])) <= 1e-12, n


def test_ssim_restatement_rejects_small_images():
    with pytest.raises(ValueError):
        R.ssim(np.zeros((6, 10, 3)), np.zeros((6, 10, 3)))


def test_ssim_skimage_inputs_regenerate():
    z = np.load(os.path.join(GOLDEN, "ssim_skimage.npz"))
    cases = RS.make_cases()
    assert sorted(cases) == _cases(z)
    for n, (x, y, mask) in cases.items():
        np.testing.assert_array_equal(x, z[n + "/x"])
        np.testing.assert_array_equal(y, z[n + "/y"])
        np.testing.assert_array_equal(mask, z[n + "/mask"])


def test_eval_metric_recorder_inputs_regenerate():
    from tests.golden import record_eval_metrics as RE
    z = np.load(os.path.join(GOLDEN, "pixel_source_features.npz"))
    dyn, feats = RE.pixel_source_inputs(**RE.PIXEL_SOURCE_FEATURES)
    np.testing.assert_array_equal(dyn.numpy(), z["src/dynamic_masks"])
    np.testing.assert_array_equal(feats.numpy(), z["src/features"])
    z = np.load(os.path.join(GOLDEN, "render_pixels_feature.npz"))
    images = RE.render_pixels_feature_images(**RE.RENDER_PIXELS_FEATURE)
    for i, d in enumerate(images):
        for k, v in d.items():
            np.testing.assert_array_equal(v.numpy(), z[f"image{i}/{k}"], err_msg=f"image{i}/{k}")
    zero = RE.RENDER_PIXELS_FEATURE["zero_mask_image"]
    assert not z[f"image{zero}/dynamic_masks"].any() and all(z[f"image{i}/dynamic_masks"].any() for i in range(3) if i != zero)
