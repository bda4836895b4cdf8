"""Device SSIM, squared-error sums, the pixel-source extras gather and the eval loop's six metrics (csrc/metrics.hip,
csrc/rays.hip emer_gather_pixel_extras, emernerf_amd/video_utils.py) against scikit-image's own recording, float64 numpy and
recordings of the reference's pixel source and render loop (tests/golden/record_*.py)."""
import os

import numpy as np
import pytest
import torch

from tests import _ssim_ref as R
from tests.golden import make_golden as G
from tests.golden import record_eval_metrics as RE

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DEV = torch.device("cuda:0")


def _ssim_dev(x, y, mask=None, full=True):
    from emernerf_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    res = ops.ssim(t(x), t(y), None if mask is None else t(mask), full=full)
    if full:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


def _check_against_f64(x, y, mask, tag):
    out, S = _ssim_dev(x, y, mask)
    s_ref, S_ref = R.ssim(x, y, full=True)
    S_ref = S_ref.reshape(S.shape)
    assert np.abs(S - S_ref).max() <= 1e-5, f"{tag}: map err {np.abs(S - S_ref).max():.2e}"
    assert abs(out[0] - s_ref) <= 1e-7, f"{tag}: ssim err {abs(out[0] - s_ref):.2e}"
    m = mask.reshape(S.shape[:2]).astype(bool)
    assert out[2] == m.sum() * S.shape[2], tag
    if m.any():
        assert abs(out[1] / out[2] - R.masked_ssim(x, y, mask)) <= 1e-7, tag
    else:
        assert out[1] == 0.0


def test_ssim_matches_skimage_recording(hip_lib):
    """ops.ssim vs scikit-image itself (tests/golden/ssim_skimage.npz): S map 1e-5 per entry, scalar and masked mean 1e-7 --
    including the bright flat case (where fp32 moments fail) and constant regions (zero variance)."""
    z = np.load(os.path.join(GOLDEN, "ssim_skimage.npz"))
    names = sorted({k.split("/")[0] for k in z.files if "/" in k})
    assert "bright_flat" in names and "constant" in names
    for n in names:
        x, y, mask = z[n + "/x"], z[n + "/y"], z[n + "/mask"]
        out, S = _ssim_dev(x, y, mask)
        want = z[n + "/map"].reshape(S.shape)
        assert np.abs(S - want).max() <= 1e-5, f"{n}: map err {np.abs(S - want).max():.2e}"
        assert abs(out[0] - float(z[n + "/ssim"])) <= 1e-7, n
        assert abs(out[1] / out[2] - float(z[n + "/masked_ssim"])) <= 1e-7, n


def test_ssim_large_and_ragged_shapes(hip_lib):
    """960 x 640 x 3 with a sparse mask, and shapes that are not multiples of the 32 x 16 tile, vs the float64 restatement."""
    rng = np.random.default_rng(7)
    for shape, density in (((960, 640, 3), 0.01), ((7, 300, 3), 0.3), ((301, 7, 3), 0.3), ((129, 257, 3), 0.2), ((33, 17, 1), 0.5)):
        x = rng.random(shape).astype(np.float32)
        y = np.clip(x + 0.2 * rng.standard_normal(shape), 0, 1).astype(np.float32)
        mask = rng.random(shape[:2]) < density
        _check_against_f64(x, y, mask, str(shape))
    # no mask: count 0; a uint8 [H, W, 1] mask is accepted as well
    x = rng.random((40, 50, 3)).astype(np.float32)
    out = _ssim_dev(x, x, None, full=False)
    assert abs(out[0] - 1.0) <= 1e-12 and out[1] == 0 and out[2] == 0
    m8 = (rng.random((40, 50, 1)) < 0.5).astype(np.uint8)
    _check_against_f64(x, np.clip(x + 0.05, 0, 1).astype(np.float32), m8, "uint8 mask")


def test_ssim_bitwise_stable_and_rejects_small_images(hip_lib):
    from emernerf_amd import _lib, ops
    g = torch.Generator().manual_seed(3)
    x = torch.rand(480, 640, 3, generator=g).to(DEV)
    y = (x + 0.1 * torch.randn(480, 640, 3, generator=g).to(DEV)).clamp(0, 1)
    mask = (torch.rand(480, 640, generator=g) < 0.1).to(DEV)
    slots = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    maps = []
    for i in range(4):
        maps.append(ops.ssim(x, y, mask, out=slots[i], full=True)[1])
    s = slots.cpu().numpy()
    assert (s == s[0]).all(), s
    assert all(torch.equal(maps[0], m) for m in maps[1:])
    with pytest.raises(_lib.EmerError, match="7 x 7"):
        ops.ssim(torch.rand(6, 10, 3, device=DEV), torch.rand(6, 10, 3, device=DEV))
    with pytest.raises(_lib.EmerError, match="7 x 7"):
        ops.ssim(torch.rand(10, 6, 3, device=DEV), torch.rand(10, 6, 3, device=DEV))


@pytest.mark.parametrize("E", [3, 16, 64, 768])
def test_sq_err_sums_vs_float64(hip_lib, E):
    from emernerf_amd import ops
    rng = np.random.default_rng(E)
    rows = 4097
    p = rng.random((rows, E)).astype(np.float32)
    t = rng.random((rows, E)).astype(np.float32)
    d2 = (p.astype(np.float64) - t.astype(np.float64)) ** 2
    for name, mask in (("none", None), ("empty", np.zeros(rows, bool)), ("full", np.ones(rows, bool)),
                       ("sparse", rng.random(rows) < 0.03)):
        out = ops.sq_err_sums(torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV),
                              None if mask is None else torch.from_numpy(mask).to(DEV)).cpu().numpy()
        np.testing.assert_allclose(out[0], d2.sum(), rtol=1e-12, err_msg=name)
        m = np.zeros(rows, bool) if mask is None else mask
        np.testing.assert_allclose(out[1], d2[m].sum(), rtol=1e-12, atol=0, err_msg=name)
        assert out[2] == m.sum(), name
    # ragged total (rows * cols % 4 != 0) and an offset view (no 16-byte alignment): the scalar path
    pt, tt = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    mk = torch.from_numpy(rng.random(rows) < 0.5).to(DEV)
    out = ops.sq_err_sums(pt[1:], tt[1:], mk[1:]).cpu().numpy()
    np.testing.assert_allclose(out[0], d2[1:].sum(), rtol=1e-12)
    np.testing.assert_allclose(out[1], d2[1:][mk[1:].cpu().numpy()].sum(), rtol=1e-12)


def test_pixel_source_extras_match_reference_recording(hip_lib):
    """PixelSource(dynamic_masks=..., features=...) vs the reference's ScenePixelSource (tests/golden/pixel_source_features.npz):
    key sets of get_train_rays / get_render_rays, and the gathered masks and feature rows bit for bit -- at W = 640 the 7/20
    feature scale truncates differently in float32 and float64 (x = 180, 340, 360 of the render image)."""
    from emernerf_amd.pixel_source import PixelSource
    z = np.load(os.path.join(GOLDEN, "pixel_source_features.npz"))
    dyn = torch.from_numpy(z["src/dynamic_masks"]).to(DEV)          # bool: stored as float like the reference
    feats = torch.from_numpy(z["src/features"]).to(DEV)
    n, H, W = dyn.shape
    src = PixelSource(torch.zeros(n, H, W, 3, device=DEV), torch.eye(4, device=DEV).repeat(n, 1, 1), torch.eye(3, device=DEV).repeat(n, 1, 1),
                      torch.zeros(n, H, W, device=DEV), torch.arange(n, device=DEV).float() / (n - 1), torch.zeros(n, dtype=torch.long, device=DEV),
                      dynamic_masks=dyn, features=feats)
    pc = z["train/pixel_coords"]
    y, x = np.rint(pc[:, 0] * H).astype(np.int64), np.rint(pc[:, 1] * W).astype(np.int64)
    got = src._gather(torch.from_numpy(z["train/img_idx"]).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(x).to(DEV))
    assert sorted(got) == sorted(z["train/keys"].tolist())
    for k in ("dynamic_masks", "features"):
        a, b = got[k].cpu().numpy(), z["train/" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=k)
    batch = src.get_train_rays(512)
    assert sorted(batch) == sorted(z["train/keys"].tolist()) and batch["features"].shape == (512, feats.shape[-1])
    rr = src.get_render_rays(int(z["render/img"]))
    assert sorted(rr) == sorted(z["render/keys"].tolist())
    for k in ("dynamic_masks", "features"):
        a, b = rr[k].cpu().numpy(), z["render/" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=k)


def test_pixel_source_extras_scalar_path_and_synthetic(hip_lib):
    """Feature rows whose width is not a multiple of 4 (scalar copies) vs a numpy gather; the synthetic source's new draws come
    after the old ones (the data without them is unchanged)."""
    from emernerf_amd.pixel_source import PixelSource
    src = PixelSource.synthetic(DEV, num_imgs=4, height=24, width=40, seed=5, dynamic_ratio=0.2, feature_dim=6, feature_hw=(7, 9))
    old = PixelSource.synthetic(DEV, num_imgs=4, height=24, width=40, seed=5)
    assert torch.equal(src.images, old.images) and torch.equal(src.sky_masks, old.sky_masks)
    assert old.dynamic_masks is None and old.features is None
    b = src.get_train_rays(1000)
    img, pc = b["img_idx"].cpu().numpy(), b["pixel_coords"].cpu().numpy()
    y, x = np.rint(pc[:, 0] * 24).astype(np.int64), np.rint(pc[:, 1] * 40).astype(np.int64)
    fy = (y.astype(np.float32) * np.float32(7 / 24)).astype(np.int64)
    fx = (x.astype(np.float32) * np.float32(9 / 40)).astype(np.int64)
    np.testing.assert_array_equal(b["features"].cpu().numpy(), src.features.cpu().numpy()[img, fy, fx])
    np.testing.assert_array_equal(b["dynamic_masks"].cpu().numpy(), src.dynamic_masks.cpu().numpy()[img, y, x])
    assert "dynamic_masks" not in old.get_train_rays(16) and "features" not in old[0]


def _render_feature_case():
    from emernerf_amd.prop_net import PropNetEstimator
    from emernerf_amd.radiance_field import build_density_field, build_radiance_field_from_cfg
    gold = np.load(os.path.join(GOLDEN, "render_pixels_feature.npz"))
    cfg = G.model_cfg("feature")
    torch.manual_seed(0)
    model = build_radiance_field_from_cfg(cfg, verbose=False)
    props = [build_density_field(aabb=G.AABB, unbounded=True, **k) for k in G.PROP_KW]
    seed = int(gold["table_seed"])
    for prefix, m in [("model/", model)] + [(f"prop{i}/", p) for i, p in enumerate(props)]:
        sd = {k: (G.table_values(prefix + k, v.numel(), seed) if k.endswith("tcnn_encoding.params")
                  else torch.from_numpy(gold["state/" + prefix + k])) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        m.to(DEV)
    model.time_diff = 1 / cfg.num_train_timesteps
    est = PropNetEstimator(None, None).to(DEV)
    n_img = RE.RENDER_PIXELS_FEATURE["n_images"]
    images = [{k[len(f"image{i}/"):]: torch.from_numpy(v).to(DEV) for k, v in gold.items() if k.startswith(f"image{i}/")} for i in range(n_img)]
    return gold, model, props, est, images


def test_render_pixels_metrics_match_reference_loop(hip_lib):
    """render_pixels(compute_metrics=True) on the feature model vs the reference's loop (tests/golden/render_pixels_feature.npz):
    the six scalars (psnr-type at rtol 1e-4; ssim-type within 1e-3: the rendered pixels differ by up to 2e-5), and the same
    scalars recomputed in float64 from the loop's OWN returned images to 1e-6, which pins crop, mask and the exclusion of the
    image whose mask is empty.  compute_metrics=False: all six are -1."""
    from emernerf_amd.video_utils import render_pixels
    gold, model, props, est, images = _render_feature_case()
    rcfg = G.render_cfg([24, 16], 16, chunk=64)
    out = render_pixels(rcfg, model, est, G.GoldenSplit(images), proposal_networks=props, compute_metrics=True, return_decomposition=True)
    for k in ("psnr", "feat_psnr", "masked_psnr", "masked_feat_psnr"):
        np.testing.assert_allclose(out[k], float(gold["scalar/" + k]), rtol=1e-4, err_msg=k)
    for k in ("ssim", "masked_ssim"):
        assert abs(out[k] - float(gold["scalar/" + k])) <= 1e-3, (k, out[k], float(gold["scalar/" + k]))
    # float64 restatement on the loop's own images
    zero = RE.RENDER_PIXELS_FEATURE["zero_mask_image"]
    ssims, mssims, mpsnrs = [], [], []
    for j, d in enumerate(images):
        rgb, gt = out["rgbs"][j].astype(np.float64), out["gt_rgbs"][j].astype(np.float64)
        m = d["dynamic_masks"].cpu().numpy().astype(bool)
        ssims.append(R.ssim(rgb, gt))
        if m.any():
            mssims.append(R.masked_ssim(rgb, gt, m))
            mpsnrs.append(-10 * np.log10(((rgb[m] - gt[m]) ** 2).mean()))
        else:
            assert j == zero
    assert len(mssims) == len(images) - 1
    assert abs(out["ssim"] - np.mean(ssims)) <= 1e-6
    assert abs(out["masked_ssim"] - np.mean(mssims)) <= 1e-6
    assert abs(out["masked_psnr"] - np.mean(mpsnrs)) <= 1e-4
    off = render_pixels(rcfg, model, est, G.GoldenSplit(images), proposal_networks=props, compute_metrics=False, return_decomposition=True)
    for k in ("psnr", "ssim", "feat_psnr", "masked_psnr", "masked_ssim", "masked_feat_psnr"):
        assert off[k] == -1, k


def test_render_without_masks_or_features_keeps_minus_one(hip_lib):
    """A split without dynamic_masks / features: ssim is computed, the four masked / feature metrics stay -1."""
    from emernerf_amd.pixel_source import PixelSource
    from emernerf_amd.trainer import Trainer, render_config
    from emernerf_amd.video_utils import render_pixels
    tr = Trainer(kind="dynamic", device=DEV, num_samples=32, prop_samples=(32, 16), table_init=0.3, seed=2)
    src = PixelSource.synthetic(DEV, num_imgs=3, height=24, width=40, seed=1)
    out = render_pixels(render_config(32, (32, 16), chunk=512), tr.model, tr.estimator, src, proposal_networks=tr.props,
                        compute_metrics=True)
    want = np.mean([R.ssim(a.astype(np.float64), b.astype(np.float64)) for a, b in zip(out["rgbs"], out["gt_rgbs"])])
    assert abs(out["ssim"] - want) <= 1e-6
    for k in ("feat_psnr", "masked_psnr", "masked_ssim", "masked_feat_psnr"):
        assert out[k] == -1, k


def test_feature_trainer_step_from_pixel_source(hip_lib):
    """A feature model (BASELINE configs[4]) trained from the project's own ray source: PixelSource batches carry 64-d features,
    and the step's loss includes the feature term (finite, and larger than the same step without the features)."""
    from emernerf_amd.pixel_source import PixelSource
    from emernerf_amd.trainer import Trainer
    src = PixelSource.synthetic(DEV, num_imgs=6, height=32, width=48, num_cams=3, seed=4, dynamic_ratio=0.1, feature_dim=64)
    batch = src.get_train_rays(512)
    assert batch["features"].shape == (512, 64) and batch["dynamic_masks"].shape == (512,)
    losses = []
    for with_feat in (True, False):
        tr = Trainer(kind="feature", device=DEV, num_samples=32, prop_samples=(32, 16), table_init=0.2, seed=1)
        data = dict(batch) if with_feat else {k: v for k, v in batch.items() if k != "features"}
        losses.append(float(tr.train_step(data)["loss"]))
    assert np.isfinite(losses).all() and losses[0] > losses[1], losses
