"""GPU tests of the low-resolution render path (csrc/rays.hip render_rays_lowres_kernel, PixelSource.update_downscale_factor),
the on-device refresh of the pixel error buffer (pixel_error_image_kernel / pixel_error_normalise_kernel) and their driver
(video_utils.cache_pixel_error_maps), against the recording of the reference's own ScenePixelSource
(tests/golden/pixel_source_lowres.npz) and the double-precision restatement and derived bounds of tests/_resample_ref.py."""
import os

import numpy as np
import pytest
import torch

from tests import _resample_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"A": ((37, 53), 1 / 4, (9, 13)), "B": ((37, 53), 1 / 3, (12, 17)), "C": ((100, 72), 1 / 16, (6, 4))}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "pixel_source_lowres.npz"))


def _source(gold, case, **kw):
    from emernerf_amd.pixel_source import PixelSource
    tag = str(gold[f"{case}/source"])
    t = {k.split("/", 1)[1]: torch.from_numpy(gold[k]).to(DEV) for k in gold.files if k.startswith(f"src{tag}/")}
    return PixelSource(t["images"], t["cam_to_worlds"], t["intrinsics"], t["sky_masks"], t["normalized_timestamps"], t["cam_ids"],
                       dynamic_masks=t["dynamic_masks"], features=t["features"], **kw)


def _bits(d):
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_rays_match_the_reference_recording(hip_lib, gold, case):
    """get_render_rays at factors 1/4, 1/3 and 1/16 for images 0..2: the recording's key set, shapes and dtypes; origins,
    pixel_coords, masks, features, ids and timestamps bit for bit; viewdirs / direction_norm at 2e-7; pixels within
    c_resample * 2^-24 * abs_sum of the float64 restatement per entry (abs_sum = 0: exactly 0)."""
    hw, s, out_hw = CASES[case]
    src = _source(gold, case)
    assert src.downscale_factor == 1.0
    src.update_downscale_factor(s)
    assert src.downscale_factor == s
    images = gold[f"src{gold[f'{case}/source']}/images"]
    for i in range(3):
        rr = _bits(src.get_render_rays(i))
        assert sorted(rr) == list(gold[f"{case}/keys"])
        for k, a in rr.items():
            b = gold[f"{case}/img{i}/{k}"]
            assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
            if k in ("viewdirs", "direction_norm"):
                np.testing.assert_allclose(a, b, rtol=2e-7, atol=2e-7, err_msg=f"{case} image {i} {k}")
            elif k != "pixels":
                np.testing.assert_array_equal(a, b, err_msg=f"{case} image {i} {k}")
        assert rr["pixels"].shape == (*out_hw, 3)
        r = R.resample(images[i], s)
        err = np.abs(rr["pixels"].astype(np.float64) - r["ref"])
        bound = R.c_resample(r["ny"], r["nx"]) * R.U * r["abs_sum"]
        pos = r["abs_sum"] > 0
        print(f"case {case} image {i}: worst {float((err[pos] / (R.U * r['abs_sum'][pos])).max()):.2f} * 2^-24 * abs_sum "
              f"(bound {float(R.c_resample(r['ny'], r['nx']).max()):.0f}); vs the recording {np.abs(rr['pixels'] - gold[f'{case}/img{i}/pixels']).max():.2e}")
        assert (err <= bound).all(), f"{case} image {i}: {float((err[pos] / bound[pos]).max()):.2f} x the bound"
        assert (rr["pixels"][~pos] == 0).all()


def test_reset_and_factor_one_are_the_full_resolution_path(hip_lib, gold):
    src = _source(gold, "A")
    before = _bits(src.get_render_rays(1))
    train_before = _bits(src._gather(*(torch.tensor(v, device=DEV) for v in ([2, 0], [36, 5], [52, 7]))))
    src.update_downscale_factor(1 / 4)
    assert src.get_render_rays(1)["pixels"].shape == (9, 13, 3)
    train_low = _bits(src._gather(*(torch.tensor(v, device=DEV) for v in ([2, 0], [36, 5], [52, 7]))))   # not affected by the factor
    src.reset_downscale_factor()
    assert src.downscale_factor == 1.0
    after = _bits(src.get_render_rays(1))
    src.update_downscale_factor(1.0)
    one = _bits(src.get_render_rays(1))
    assert list(before) == list(after) == list(one)
    for k in before:
        assert before[k].shape[:2] == (37, 53)
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
        np.testing.assert_array_equal(before[k], one[k], err_msg=k)
    for k in train_before:
        np.testing.assert_array_equal(train_before[k], train_low[k], err_msg=k)
    # update remembers one previous value, reset restores it (the reference's semantics)
    src.update_downscale_factor(0.5)
    src.update_downscale_factor(0.25)
    src.reset_downscale_factor()
    assert src.downscale_factor == 0.5


def test_error_buffer_refresh_on_the_recorded_lists(hip_lib, gold):
    """accumulate_pixel_error + finish_pixel_error_maps vs update_pixel_error_maps in float64, within the bound derived in
    _resample_ref.pixel_error_ref (4 roundings for the mean of three, 1 for the x 5, 3 for the normalisation); the minimum cell
    exactly 0, the maximum 1 within 1 ulp; the recorded reference inside the same bound; same storage; support count renewed."""
    src = _source(gold, "A", buffer_ratio=0.5, buffer_downscale=4)
    src.build_pixel_error_buffer()
    assert tuple(src.pixel_error_maps.shape) == (3, 9, 13)
    assert src._support_ok(351) and not src.pixel_error_buffered
    ptr, maps = src.pixel_error_maps.data_ptr(), src.pixel_error_maps
    pred, gt, opa = (torch.from_numpy(gold[f"error/{k}"]).to(DEV) for k in ("rgbs", "gt_rgbs", "dynamic_opacities"))
    with pytest.raises(RuntimeError):
        src.accumulate_pixel_error(0, pred[0], gt[0], opa[0])
        src.finish_pixel_error_maps()          # images 1 and 2 are missing
    for i in range(3):
        src.accumulate_pixel_error(i, pred[i], gt[i], opa[i])
    src.finish_pixel_error_maps()
    assert src.pixel_error_maps is maps and maps.data_ptr() == ptr and src.pixel_error_buffered
    got = maps.cpu().numpy().astype(np.float64)
    v, bound = R.pixel_error_ref(gold["error/rgbs"], gold["error/gt_rgbs"], gold["error/dynamic_opacities"])
    print(f"refresh: worst {float((np.abs(got - v) / bound).max()):.3f} of the bound; the recording {float((np.abs(gold['error/maps'] - v) / bound).max()):.3f}")
    assert (np.abs(got - v) <= bound).all()
    assert (np.abs(gold["error/maps"].astype(np.float64) - v) <= bound).all()
    assert got.min() == 0.0 and got.reshape(-1)[v.argmin()] == 0.0
    assert abs(got.max() - 1.0) <= 2.0 ** -23 and got.reshape(-1).argmax() == v.argmax()
    n_pos = int((v > 0).sum())
    assert n_pos == 350
    assert src._support_ok(n_pos) and not src._support_ok(n_pos + 1)
    # without opacities: no x 5
    for i in range(3):
        src.accumulate_pixel_error(i, pred[i].reshape(-1, 3), gt[i].reshape(-1, 3))
    src.finish_pixel_error_maps()
    v2, bound2 = R.pixel_error_ref(gold["error/rgbs"], gold["error/gt_rgbs"])
    assert (np.abs(maps.cpu().numpy() - v2) <= bound2).all() and maps.data_ptr() == ptr


@pytest.fixture(scope="module")
def end_to_end(hip_lib):
    """cache_pixel_error_maps on a synthetic source and a toy-grid dynamic model, then render_pixels at the same factor."""
    from emernerf_amd.pixel_source import PixelSource
    from emernerf_amd.trainer import Trainer, render_config
    from emernerf_amd.video_utils import cache_pixel_error_maps, render_pixels
    tr = Trainer(kind="dynamic", device=DEV, num_samples=32, prop_samples=(32, 16), table_init=0.3, seed=2)
    cfg = render_config(32, (32, 16), chunk=40)      # 63 rays per image: two chunks
    mk = lambda: PixelSource.synthetic(DEV, num_imgs=4, height=28, width=36, seed=3, buffer_ratio=0.5, dynamic_ratio=0.2)
    src = mk()
    src.build_pixel_error_buffer()
    ptr = src.pixel_error_maps.data_ptr()
    modules = [tr.model, tr.estimator, *tr.props]
    tr.model.train(), tr.estimator.train()
    for j, p in enumerate(tr.props):
        p.train(j % 2 == 0)
    modes = [m.training for m in modules]
    cache_pixel_error_maps(cfg, tr.model, tr.estimator, src, tr.props)
    state = dict(modes_before=modes, modes_after=[m.training for m in modules], factor_after=src.downscale_factor, same_ptr=src.pixel_error_maps.data_ptr() == ptr)
    src.update_downscale_factor(1 / 4)
    out = render_pixels(cfg, tr.model, tr.estimator, src, proposal_networks=tr.props, compute_metrics=True)
    src.reset_downscale_factor()
    return src, mk, out, state


def test_cache_pixel_error_maps_end_to_end(end_to_end):
    src, mk, out, state = end_to_end
    assert state["modes_after"] == state["modes_before"] and state["factor_after"] == 1.0 and state["same_ptr"]
    assert src.pixel_error_buffered
    maps = src.pixel_error_maps.cpu().numpy()
    assert maps.shape == (4, 7, 9) and maps.min() == 0.0 and maps.max() <= 1.0 and np.isfinite(maps).all()
    # the buffer is the refresh applied to what render_pixels returns at the same factor (the forward kernels are deterministic)
    ref = mk()
    ref.build_pixel_error_buffer()
    assert len(out["dynamic_opacities"]) == 4
    for i in range(4):
        ref.accumulate_pixel_error(i, *(torch.from_numpy(np.ascontiguousarray(out[k][i])).to(DEV) for k in ("rgbs", "gt_rgbs", "dynamic_opacities")))
    ref.finish_pixel_error_maps()
    np.testing.assert_array_equal(ref.pixel_error_maps.cpu().numpy(), maps)
    # the sampler reads the new weights: the zero-weight cell is never drawn by the importance half of a batch
    zero = np.argwhere(maps == 0.0)
    assert len(zero) == 1
    assert src._support_ok(251) and not src._support_ok(252)
    hit = False
    for _ in range(20):
        b = src.get_train_rays(64)
        img = b["img_idx"][32:].cpu().numpy()
        pc = b["pixel_coords"][32:].cpu().numpy()
        y, x = np.rint(pc[:, 0] * 28).astype(np.int64), np.rint(pc[:, 1] * 36).astype(np.int64)
        hit |= bool(((img == zero[0, 0]) & (y // 4 == zero[0, 1]) & (x // 4 == zero[0, 2])).any())
    assert not hit


def test_render_pixels_low_resolution_preview(end_to_end):
    """render_pixels / render need nothing but the smaller images: 28 x 36 at factor 1/4 -> 7 x 9 previews with metrics."""
    _, _, out, _ = end_to_end
    assert len(out["rgbs"]) == len(out["gt_rgbs"]) == 4
    for a, b in zip(out["rgbs"], out["gt_rgbs"]):
        assert a.shape == (7, 9, 3) and b.shape == (7, 9, 3)
    assert np.isfinite(out["psnr"]) and out["psnr"] > 0
    assert np.isfinite(out["ssim"])      # 7 x 9 is not below the 7 x 7 window
