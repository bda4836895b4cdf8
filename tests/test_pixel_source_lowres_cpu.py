"""CPU tests of the low-resolution render path's yardsticks (no GPU, no kernel): the recording of the reference's
``get_render_rays`` at a downscale factor (tests/golden/pixel_source_lowres.npz, written by record_pixel_source_lowres.py)
against the double-precision restatement of tests/_resample_ref.py, which the GPU tests then hold the kernel to."""
import os

import numpy as np
import pytest

from tests import _resample_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"A": ((37, 53), 1 / 4, (9, 13)), "B": ((37, 53), 1 / 3, (12, 17)), "C": ((100, 72), 1 / 16, (6, 4))}
IMPULSE_IMAGE = 1


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "pixel_source_lowres.npz"))


def _source(gold, case):
    tag = str(gold[f"{case}/source"])
    return {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith(f"src{tag}/")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_recording_has_the_stated_cases(gold, case):
    hw, s, out_hw = CASES[case]
    assert float(gold[f"{case}/factor"]) == s
    assert _source(gold, case)["images"].shape[1:3] == hw
    assert (R.out_size(hw[0], s), R.out_size(hw[1], s)) == out_hw
    for i in range(3):
        assert gold[f"{case}/img{i}/pixels"].shape == (*out_hw, 3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_recorded_colours_lie_within_the_derived_bound_of_the_restatement(gold, case):
    """Entry by entry: |recording - fp64 restatement| <= c_torch_separable * 2^-24 * abs_sum; abs_sum = 0 -> exactly 0."""
    _, s, _ = CASES[case]
    images = _source(gold, case)["images"]
    worst = 0.0
    for i in range(3):
        r = R.resample(images[i], s)
        got = gold[f"{case}/img{i}/pixels"].astype(np.float64)
        err, bound = np.abs(got - r["ref"]), R.c_torch_separable(r) * R.U * r["abs_sum"]
        pos = r["abs_sum"] > 0
        worst = max(worst, float((err[pos] / (R.U * r["abs_sum"][pos])).max()))
        assert (err <= bound).all(), f"{case} image {i}: {float((err / np.maximum(bound, 1e-300)).max()):.2f} x the bound"
        assert (got[~pos] == 0).all()
    print(f"case {case}: the reference's worst error is {worst:.2f} * 2^-24 * abs_sum")


@pytest.mark.parametrize("case", sorted(CASES))
def test_nearest_index_reproduces_the_recorded_masks(gold, case):
    hw, s, _ = CASES[case]
    src = _source(gold, case)
    iy, ix = R.nearest_index(hw[0], s), R.nearest_index(hw[1], s)
    for i in range(3):
        for k in ("sky_masks", "dynamic_masks"):
            np.testing.assert_array_equal(gold[f"{case}/img{i}/{k}"], src[k][i][iy][:, ix], err_msg=f"{case} image {i} {k}")


@pytest.mark.parametrize("mutant", [dict(mapping="in/out"), dict(a=-0.75), dict(renormalise=False)], ids=["scale_in_over_out", "a_-0.75", "no_border_renorm"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_impulse_image_discriminates_the_mutants(gold, case, mutant):
    """A restatement with the mapping scale H / h instead of 1 / s, with a = -0.75, or without border renormalisation puts the
    recording of the impulse image outside the bound that the true restatement keeps it in."""
    _, s, _ = CASES[case]
    image = _source(gold, case)["images"][IMPULSE_IMAGE]
    got = gold[f"{case}/img{IMPULSE_IMAGE}/pixels"].astype(np.float64)
    r = R.resample(image, s, **mutant)
    err, bound = np.abs(got - r["ref"]), R.c_torch_separable(r) * R.U * r["abs_sum"]
    assert (err > bound).any(), f"{case}: the impulse image does not tell {mutant} from the filter"
    assert float((err - bound).max()) > 1e-4    # and by far more than rounding


def test_recorded_error_maps_lie_within_the_bound(gold):
    v, bound = R.pixel_error_ref(gold["error/rgbs"], gold["error/gt_rgbs"], gold["error/dynamic_opacities"])
    got = gold["error/maps"].astype(np.float64)
    assert got.shape == (3, 9, 13)
    assert (np.abs(got - v) <= bound).all()
    assert got.min() == 0.0 and abs(got.max() - 1.0) <= 2.0 ** -23
    assert (gold["error/dynamic_opacities"] > 0.1).mean() > 0.2
