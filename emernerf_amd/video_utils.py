"""Evaluation render loop on the HIP kernels.

Mirrors the rendering half of the reference's radiance_fields/video_utils.py: ``render_pixels`` (:50-106) and ``render``
(:109-468) -- iterate over the images of a split, call ``render_rays`` in eval mode with ``return_decomposition`` on
16 384-ray chunks (cfg.render.render_chunk_size), and collect per-image outputs under the reference's key names (rgbs,
gt_rgbs, depths, opacities, static_* / dynamic_* decomposition, shadow_reduced_static_rgbs, flows, sky_masks ...).

What changed underneath: an image's rays come from ``PixelSource.get_render_rays`` (one gather kernel), all chunks of an
image are rendered before any result leaves the GPU, an image's results leave it as ONE asynchronous transfer that overlaps
the next image's rendering (the reference interleaves a blocking ``.cpu().numpy()`` per key with the rendering), and the
metrics -- PSNR, SSIM (scikit-image's algorithm, csrc/metrics.hip), feature PSNR and their dynamic-mask variants -- are
computed on the device and read back once after the loop.  ``cache_pixel_error_maps`` is the training loop's periodic
refresh of the importance sampler's error buffer (train_emernerf.py:879-904): a low-resolution pass over the full set whose
results never leave the GPU.

``visualize=True`` adds the reference's pictures (video_utils.py:184-187,233-418): ``forward_flows`` / ``backward_flows`` become the
colour-wheel images and a feature model's DINO lists (``dino_feats``, ``gt_dino_feats``, ``dino_feats_pe_free``, ``dino_pe``,
``static_dino_feats``, ``dynamic_dino_feats`` and the two cross blends) are produced from the E-wide feature images by the
kernels of csrc/colours.hip: at most two launches per image for all feature lists, one for the flows; only [H, W, 3] colours
join the image's transfer.  ``get_robust_pca`` is the reference's robust PCA colour rule (utils/misc.py:23-47) made
deterministic.

``save_videos`` / ``save_concatenated_videos`` / ``save_seperate_videos`` (video_utils.py:471-627) turn the lists into the
8-bit frames the reference logs and writes: ``compose_video_frames`` builds each merged frame -- the keys' rows, the turbo
depth colouring, the cut to 8 bits -- in ONE launch of csrc/frames.hip, so that with ``render(..., to_host=False)`` only
3 bytes per frame pixel leave the GPU.  Out of scope here: the video encoding itself (imageio's, or the caller's writer),
the weighted-percentile depth bounds inside a merged frame (the loop passes 4 / 120 as the reference's does; one image's own
bounds are ``ops.depth_colours(depth, opacity, "auto", "auto")``).  The reference's ``resize_five_views`` -- the two outer views
of a five-camera frame shrunk by a cubic-spline zoom -- is the second launch of such a frame and is asked for by name
(``five_view_resize="zoom"``).
"""
from __future__ import annotations

import logging
import time
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from .prop_net import PropNetEstimator
from .radiance_field import DensityField, RadianceField
from .render_utils import render_rays

logger = logging.getLogger()

# results key -> (list name in the returned dict)  (video_utils.py:118-146)
_COLLECT = {"rgb": "rgbs", "static_rgb": "static_rgbs", "shadow_reduced_static_rgb": "shadow_reduced_static_rgbs",
            "shadow_only_static_rgb": "shadow_only_static_rgbs", "depth": "depths", "opacity": "opacities",
            "static_depth": "static_depths", "static_opacity": "static_opacities", "dynamic_depth": "dynamic_depths",
            "dynamic_opacity": "dynamic_opacities", "forward_flow": "forward_flows", "backward_flow": "backward_flows"}


def compute_psnr(prediction: Tensor, target: Tensor) -> float:
    """datasets/metrics.py:31-46."""
    return float(-10.0 * torch.log10(torch.nn.functional.mse_loss(prediction, target)))


def _pack_to_host(keep: Dict[str, Tensor], pinned: Dict[int, Tensor], slot: int):
    """Start the transfer of one image's results: (names, shapes, dtypes, host buffer, event)."""
    names = list(keep)
    parts = [keep[n].squeeze() for n in names]
    flat = torch.cat([p.reshape(-1).to(torch.float32) for p in parts]) if parts else None
    if flat is None:
        return names, [], [], None, None
    buf = pinned.get(slot)
    if buf is None or buf.numel() < flat.numel():
        buf = pinned[slot] = torch.empty((flat.numel(),), dtype=torch.float32, pin_memory=True)
    host = buf[:flat.numel()]
    host.copy_(flat, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return names, [tuple(p.shape) for p in parts], [p.dtype for p in parts], host, ev


def _unpack(item, out: Dict[str, list]) -> None:
    names, shapes, dtypes, host, ev = item
    if host is None:
        return
    ev.synchronize()
    arr, o = host.numpy(), 0
    for name, shape, dt in zip(names, shapes, dtypes):
        n = int(np.prod(shape)) if len(shape) else 1
        a = arr[o:o + n].reshape(shape).copy()  # the pinned buffer is reused two images later
        out[name].append(a if dt == torch.float32 else a.astype(torch.empty((), dtype=dt).numpy().dtype))
        o += n


def render_pixels(cfg, model: RadianceField, proposal_estimator: PropNetEstimator, dataset,
                  proposal_networks: Optional[List[DensityField]] = None, compute_metrics: bool = False,
                  vis_indices: Optional[List[int]] = None, return_decomposition: bool = True, visualize: bool = False,
                  feature_pca: Optional[dict] = None, to_host: bool = True) -> Dict[str, list]:
    """video_utils.py:50-106.  ``dataset``: anything with ``__len__`` / ``__getitem__`` returning image-shaped ray dicts
    (``PixelSource`` here; the reference's SplitWrapper there).  Nothing here or in ``render`` depends on the image size: with
    ``PixelSource.update_downscale_factor(1 / k)`` set, the same loop is the reference's low-resolution preview pass
    (train_emernerf.py:290-302) on [floor(H / k), floor(W / k)] images; previews smaller than 7 x 7 fall under ``render``'s
    SSIM rule.  ``visualize`` / ``feature_pca`` / ``to_host``: see ``render``."""
    model.eval()
    for p in proposal_networks or []:
        p.eval()
    if proposal_estimator is not None:
        proposal_estimator.eval()

    def render_func(data_dict):
        return render_rays(radiance_field=model, proposal_estimator=proposal_estimator, proposal_networks=proposal_networks,
                           data_dict=data_dict, cfg=cfg, return_decomposition=return_decomposition)

    results = render(dataset, render_func, model=model, compute_metrics=compute_metrics, vis_indices=vis_indices, visualize=visualize,
                     feature_pca=feature_pca, to_host=to_host)
    if compute_metrics:
        n = len(dataset) if vis_indices is None else len(vis_indices)
        logger.info(f"Eval over {n} images:")
        logger.info(f"\tPSNR: {results['psnr']:.4f}")
        logger.info(f"\tSSIM: {results['ssim']:.4f}")
        logger.info(f"\tFeature PSNR: {results['feat_psnr']:.4f}")
        logger.info(f"\tMasked PSNR: {results['masked_psnr']:.4f}")
        logger.info(f"\tMasked SSIM: {results['masked_ssim']:.4f}")
        logger.info(f"\tMasked Feature PSNR: {results['masked_feat_psnr']:.4f}")
    return results


def cache_pixel_error_maps(cfg, model: RadianceField, proposal_estimator: PropNetEstimator, pixel_source,
                           proposal_networks: Optional[List[DensityField]] = None) -> None:
    """train_emernerf.py:884-904: re-render every image at 1 / buffer_downscale of its size in eval mode and re-weight the
    importance sampler with the result.  ``render_rays`` (chunked by cfg.render.render_chunk_size) leaves ``rgb`` and
    ``dynamic_opacity`` on the device, where ``PixelSource.accumulate_pixel_error`` turns them and the resampled ground truth
    into the image's row of the error buffer; ``finish_pixel_error_maps`` normalises the buffer in place.  No host transfer,
    and the buffer keeps its storage.  The downscale factor is reset and every module's train / eval mode restored, also when
    rendering raises.  A source without an error buffer (buffer_ratio == 0) is left alone, as in the reference."""
    if pixel_source.pixel_error_maps is None:
        return
    modules = [m for m in (model, proposal_estimator, *(proposal_networks or [])) if m is not None]
    modes = [m.training for m in modules]
    for m in modules:
        m.eval()
    pixel_source.update_downscale_factor(1 / pixel_source.buffer_downscale)
    try:
        with torch.no_grad():
            for i in range(len(pixel_source)):
                data = pixel_source[i]
                res = render_rays(radiance_field=model, proposal_estimator=proposal_estimator, proposal_networks=proposal_networks,
                                  data_dict=data, cfg=cfg, return_decomposition=True)
                pixel_source.accumulate_pixel_error(i, res["rgb"], data["pixels"], res.get("dynamic_opacity"))
            pixel_source.finish_pixel_error_maps()
    finally:
        pixel_source.reset_downscale_factor()
        for m, training in zip(modules, modes):
            m.train(training)


def get_robust_pca(features: Tensor, m: float = 2.0) -> Tuple[Tensor, Tensor, Tensor]:
    """utils/misc.py:23-47 (remove_first_component=False), deterministic: (reduction matrix [E, 3], colour min [3], colour max
    [3]) of [N, E] features.  The matrix holds the three leading principal axes of the CENTRED features -- the top eigenvectors
    of the E x E covariance (float64 ``torch.linalg.eigh`` on the host: it runs once per loop), each column's sign fixed so that
    its largest-magnitude entry is positive -- where the reference's ``torch.pca_lowrank`` is randomised (same subspace, not the
    same digits).  The colours are the UNCENTRED product ``features @ matrix``; min and max per channel run over the rows whose
    absolute deviation from the channel's median is below ``m`` times the median absolute deviation.  Plain torch: works on CPU
    and device tensors."""
    assert features.dim() == 2 and features.shape[1] >= 3, "features should be (N, C) with C >= 3"
    x = features.detach().to(torch.float64)
    xc = x - x.mean(dim=0, keepdim=True)
    _, vecs = torch.linalg.eigh((xc.T @ xc).cpu())          # eigenvalues ascending
    v = vecs[:, [-1, -2, -3]]
    top = v.abs().argmax(dim=0)
    v = v * torch.sign(v[top, torch.arange(3)])
    mat = v.to(device=features.device, dtype=features.dtype)
    colors = features.detach() @ mat
    d = torch.abs(colors - torch.median(colors, dim=0).values)
    s = d / torch.median(d, dim=0).values
    lo = torch.stack([colors[s[:, c] < m, c].min() for c in range(3)])
    hi = torch.stack([colors[s[:, c] < m, c].max() for c in range(3)])
    return mat, lo.to(mat), hi.to(mat)


_FEATURE_LISTS = ["dino_feats", "gt_dino_feats", "dino_feats_pe_free", "dino_pe", "static_dino_feats", "dynamic_dino_feats",
                  "dynamic_dino_on_static_rgbs", "dynamic_rgb_on_static_dinos"]


def _feature_colour_lists(res: Dict[str, Tensor], data: Dict[str, Tensor], model, pca: Optional[dict]):
    """The reference's DINO colour lists of one image (video_utils.py:233-418), quirks included, as ({list name: [H, W, 3]
    colours}, pca): ONE launch for every projection (per feature width), ONE for the two cross blends.  ``pca``: the PE-free / PE
    matrices; computed here from this image when None and the results carry ``dino_pe_free`` (:273-301)."""
    if model is None:
        raise ValueError("render(visualize=True): the feature colours need `model` (its registered feats_reduction_mat / feat_color_min / feat_color_max)")
    feat = res["dino_feat"]
    reg = (model.feats_reduction_mat, model.feat_color_min, model.feat_color_max)
    jobs = [("dino_feats", feat, reg, None)]                     # no opacity multiply (:413-415)
    if "features" in data:
        jobs.append(("gt_dino_feats", data["features"], reg, None))
    if "dino_pe_free" in res:
        if pca is None:
            E = res["dino_pe_free"].shape[-1]
            non_sky = res["dino_pe_free"] * (~data["sky_masks"].bool().unsqueeze(-1)).to(res["dino_pe_free"])
            pca = {"pe_free": get_robust_pca(non_sky.reshape(-1, E), m=2.5), "pe": get_robust_pca(res["dino_pe"].reshape(-1, E), m=2.5)}
        free = tuple(t.to(feat.device) for t in pca["pe_free"])
        jobs.append(("dino_feats_pe_free", res["dino_pe_free"], free, res["opacity"]))
        jobs.append(("dino_pe", res["dino_pe"], tuple(t.to(feat.device) for t in pca["pe"]), None))
        if "static_dino" in res:
            jobs.append(("static_dino_feats", res["static_dino"], free, None))
        if "dynamic_dino" in res:
            jobs.append(("dynamic_dino_feats", res["dynamic_dino"], free, res["dynamic_opacity"]))
    else:
        if "static_dino" in res:
            jobs.append(("static_dino_feats", res["static_dino"], reg, None))
        if "dynamic_dino" in res:
            jobs.append(("dynamic_dino_feats", res["dynamic_dino"], reg, None))    # no opacity multiply in this branch (:400-401)
    cols: Dict[str, Tensor] = {}
    for E in sorted({j[1].shape[-1] for j in jobs}):             # one launch (ground-truth features of another width: one more)
        part = [j for j in jobs if j[1].shape[-1] == E]
        for (name, *_), c in zip(part, ops.feature_colours_multi([(f, *p, s) for _, f, p, s in part])):
            cols[name] = c
    blends = []
    if "static_dino_feats" in cols:       # dynamic rgb over the static feature colours (:334-342, :381-389)
        blends.append(("dynamic_rgb_on_static_dinos", res["dynamic_rgb"], res["dynamic_opacity"], cols["static_dino_feats"]))
    if "dynamic_dino_feats" in cols:      # in the PE branch the dynamic colours carry dynamic_opacity already: it applies twice (:355-362)
        blends.append(("dynamic_dino_on_static_rgbs", cols["dynamic_dino_feats"], res["dynamic_opacity"], res["static_rgb"]))
    if blends:
        for (name, *_), c in zip(blends, ops.blend_over_multi([b[1:] for b in blends])):
            cols[name] = c
    return cols, pca


def render(dataset, render_func: Callable, model: Optional[RadianceField] = None, compute_metrics: bool = False,
           vis_indices: Optional[List[int]] = None, visualize: bool = False, feature_pca: Optional[dict] = None,
           to_host: bool = True) -> Dict[str, list]:
    """video_utils.py:109-468: the reference's result dictionary key for key -- the nine lists it always returns (possibly
    empty), the conditional ones (gt_rgbs, gt_sky_masks, shadow_*, forward_flows / backward_flows, median_depths), the
    scalars psnr, ssim, feat_psnr, masked_psnr, masked_ssim, masked_feat_psnr under the reference's rules (:206-247,421-428):
    ssim of every image with ground truth; masked_* only for images whose ``dynamic_masks`` has a nonzero entry; feat_psnr /
    masked_feat_psnr only where the results carry ``dino_feat`` and the data ``features``; each the mean over the images that
    contributed, -1 when none did, and all -1 when ``compute_metrics`` is False.  Per-image values stay in a device tensor
    and are read back once, after the loop.  One deliberate deviation: an image smaller than 7 x 7 is left out of ssim /
    masked_ssim (a warning is logged once), where scikit-image raises.  Checked against recordings of the reference's own
    loop: tests/golden/render_pixels_*.npz.

    ``visualize=False`` (the default): ``forward_flows`` / ``backward_flows`` hold the rendered flow and no DINO colour list
    is produced.  ``visualize=True`` is the reference's picture output: the flow lists hold ``ops.flow_colours(flow, 1.0,
    "bright")`` (:35-43,184-187), and where the results carry ``dino_feat`` the loop returns ``dino_feats``, ``gt_dino_feats``
    (data with ``features``), and -- under the reference's conditions, names and quirks (:233-418,442-457) --
    ``dino_feats_pe_free``, ``dino_pe``, ``static_dino_feats``, ``dynamic_dino_feats``, ``dynamic_rgb_on_static_dinos``,
    ``dynamic_dino_on_static_rgbs``.  The PE-free / PE colour matrices come from ``feature_pca`` ({"pe_free": (mat [E, 3],
    lo [3], hi [3]), "pe": (...)}) or, when None, from the first rendered image by ``get_robust_pca`` (sky zeroed, m = 2.5);
    they are returned under ``feature_pca`` so that a later call can colour another split consistently.  ``get_robust_pca`` is
    deterministic where the reference's ``torch.pca_lowrank`` is randomised: the colours follow the reference's formulas for
    the same matrices, not its random draw.  Checked against tests/golden/flow_colours.npz / feature_colours.npz.

    ``to_host=False`` leaves the lists on the device: each holds the image's squeezed device tensors (the values and dtypes of
    the host lists) and no image is transferred; the metrics are still read back once.  ``compose_video_frames`` /
    ``save_videos`` take such lists and move 3 bytes per frame pixel instead of 4 to 12 bytes per pixel per list.  The cost is
    device memory: every kept image (4 to 12 bytes per pixel per list, for all images of the loop) stays allocated until the
    caller drops the lists."""
    always = ["rgbs", "static_rgbs", "dynamic_rgbs", "depths", "opacities", "static_depths", "static_opacities", "dynamic_depths",
              "dynamic_opacities"]
    out: Dict[str, list] = {v: [] for v in _COLLECT.values()}
    out.update({"gt_rgbs": [], "dynamic_rgbs": [], "median_depths": [], "gt_sky_masks": []})
    if visualize:
        out.update({k: [] for k in _FEATURE_LISTS})
    pca = feature_pca
    psnrs: List[Tensor] = []
    pending: list = []
    pinned: Dict[int, Tensor] = {}
    n_rays, n_images, t0 = 0, 0, time.perf_counter()
    green = None
    # per-image metrics on the device, one row per image: ssim (value, masked S sum, masked count) | colour squared-error sums
    # (all, masked, masked rows) | feature squared-error sums (same); read back once after the loop
    metrics: Optional[Tensor] = None
    ssim_rows: List[int] = []
    rgb_mask_rows: List[Tuple[int, int]] = []          # (row, colour channels)
    feat_rows: List[Tuple[int, int, int]] = []         # (row, pixels, feature dim)
    warned_small = False
    with torch.no_grad():
        indices = vis_indices if vis_indices is not None else range(len(dataset))
        for j, i in enumerate(indices):
            data = {k: (v.cuda(non_blocking=True) if isinstance(v, Tensor) and not v.is_cuda else v) for k, v in dataset[i].items()}
            res = render_func(data)
            n_rays += int(data["origins"].numel() // 3)
            keep: Dict[str, Tensor] = {}
            for k, name in _COLLECT.items():
                if k in res:
                    keep[name] = res[k]
            if "dynamic_rgb" in res:  # green-screen blend for visualisation (:169-177)
                if green is None:
                    green = torch.tensor([0.0, 177.0, 64.0], device=res["dynamic_rgb"].device) / 255.0
                keep["dynamic_rgbs"] = res["dynamic_rgb"] * res["dynamic_opacity"] + green * (1 - res["dynamic_opacity"])
            if "dynamic_depth" not in res and "median_depth" in res:
                keep["median_depths"] = res["median_depth"]
            if "pixels" in data:
                keep["gt_rgbs"] = data["pixels"]
            if "sky_masks" in data:
                keep["gt_sky_masks"] = data["sky_masks"]
            if visualize:
                flows = [k for k in ("forward_flow", "backward_flow") if k in res]
                if flows:  # both directions of the image in one launch (:184-187)
                    for k, c in zip(flows, ops.flow_colours_multi([res[k] for k in flows], 1.0, "bright")):
                        keep[_COLLECT[k]] = c
                if "dino_feat" in res:
                    cols, pca = _feature_colour_lists(res, data, model, pca)
                    keep.update(cols)
            if compute_metrics and "pixels" in data:  # stays on the device until the loop is over (no sync per image)
                psnrs.append(-10.0 * torch.log10(torch.nn.functional.mse_loss(res["rgb"], data["pixels"])))
                if metrics is None:
                    metrics = torch.zeros((len(indices), 9), dtype=torch.float64, device=res["rgb"].device)
                mask = data.get("dynamic_masks")
                H, W = res["rgb"].shape[:2]
                if H >= 7 and W >= 7:
                    ops.ssim(res["rgb"], data["pixels"], mask, out=metrics[j, 0:3])
                    ssim_rows.append(j)
                elif not warned_small:
                    logger.warning(f"render: {H} x {W} images are smaller than the 7 x 7 SSIM window; ssim / masked_ssim leave them out")
                    warned_small = True
                if mask is not None:
                    ops.sq_err_sums(res["rgb"], data["pixels"], mask, out=metrics[j, 3:6])
                    rgb_mask_rows.append((j, res["rgb"].shape[-1]))
            if compute_metrics and "dino_feat" in res and "features" in data:
                if metrics is None:
                    metrics = torch.zeros((len(indices), 9), dtype=torch.float64, device=res["dino_feat"].device)
                E = res["dino_feat"].shape[-1]
                ops.sq_err_sums(res["dino_feat"], data["features"], data.get("dynamic_masks"), out=metrics[j, 6:9])
                feat_rows.append((j, res["dino_feat"].numel() // E, E))
            # ONE device->host transfer per image: every kept tensor packed into a flat buffer, copied asynchronously into
            # pinned memory and unpacked while the NEXT image renders (the reference interleaves a blocking .cpu().numpy() per
            # key with the rendering; on a slow host that halves the loop's throughput)
            if not to_host:     # the lists stay on the device
                for name, t in keep.items():
                    out[name].append(t.squeeze())
                n_images += 1
                continue
            pending.append(_pack_to_host(keep, pinned, n_images & 1))  # two alternating pinned buffers
            n_images += 1
            if len(pending) > 1:
                _unpack(pending.pop(0), out)
        while pending:
            _unpack(pending.pop(0), out)
        # the one read-back of every metric: the psnr mean (fp32, as before) and the per-image rows
        host = None
        if psnrs or metrics is not None:
            parts = [torch.stack(psnrs).mean().double().reshape(1)] if psnrs else []
            if metrics is not None:
                parts.append(metrics.reshape(-1))
            host = torch.cat(parts).cpu().numpy()
    torch.cuda.synchronize()
    out = {k: v for k, v in out.items() if len(v) > 0 or k in always}
    dt = time.perf_counter() - t0
    out["render_rays_per_s"] = n_rays / dt if dt > 0 else float("nan")
    if visualize and pca is not None:
        out["feature_pca"] = pca
    out["psnr"] = (float(host[0]) if psnrs else -1.0) if compute_metrics else -1
    ssims, masked_ssims, masked_psnrs, feat_psnrs, masked_feat_psnrs = [], [], [], [], []
    if metrics is not None:
        m = host[len(host) - metrics.numel():].reshape(metrics.shape)
        for j in ssim_rows:
            ssims.append(float(m[j, 0]))
            if m[j, 2] > 0:   # an image whose mask has a nonzero entry
                masked_ssims.append(float(m[j, 1] / m[j, 2]))
        for j, c in rgb_mask_rows:
            if m[j, 5] > 0:
                masked_psnrs.append(_psnr(m[j, 4], m[j, 5] * c))
        for j, n, e in feat_rows:
            feat_psnrs.append(_psnr(m[j, 6], n * e))
            if m[j, 8] > 0:
                masked_feat_psnrs.append(_psnr(m[j, 7], m[j, 8] * e))
    for k, v in (("ssim", ssims), ("feat_psnr", feat_psnrs), ("masked_psnr", masked_psnrs), ("masked_ssim", masked_ssims),
                 ("masked_feat_psnr", masked_feat_psnrs)):
        out[k] = _non_zero_mean(v) if compute_metrics else -1
    return out


# ------------------------------------------------------------------------------------------------ video frames
def _frame_plan(render_results, keys, separate: bool):
    """The rows of a frame as [(key, kind, image list, opacity list | None)] under the reference's rules (video_utils.py:525-553,
    580-607): which list a key reads, which keys are skipped, what kind of tile its images become."""
    plan = []
    for key in keys:
        if separate or key != "sky_masks":      # the separate mode asks for the key itself also when it then reads the opacities (:587)
            if key not in render_results or len(render_results[key]) == 0:
                continue
        if key == "sky_masks":
            plan.append((key, "one_minus_grey1", render_results["opacities"], None))
        elif key == "gt_sky_masks":
            plan.append((key, "grey1", render_results[key], None))
        elif "depth" in key:
            name = key.replace("depths", "opacities")
            if name not in render_results:
                if separate:
                    raise KeyError(name)
                if "median" not in key:
                    continue
                name = key.replace("median_depths", "opacities")
            plan.append((key, "depth", render_results[key], render_results[name]))
        else:
            plan.append((key, "colour3", render_results[key], None))
    return plan


def _tile_image(x, kind: str, key: str, device) -> Tensor:
    """One list entry as a device tensor of the tile's shape: numpy arrays are uploaded, anything not fp32 is converted."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, Tensor):
        raise ValueError(f"{key}: list entries are numpy arrays or tensors, not {type(x).__name__}")
    ok = (t.dim() == 3 and t.shape[-1] == 3) if kind == "colour3" else t.dim() == 2
    if not ok:
        raise ValueError(f"{key}: images of shape {tuple(t.shape)} are neither [H, W, 3] colours nor one of the [H, W] cases "
                         "(gt_sky_masks, sky_masks, depths with their opacities)")
    return t.to(device=device, dtype=torch.float32, non_blocking=True)


def compose_video_frames(render_results: Dict[str, list], num_timestamps: int, keys: List[str], num_cams: int, separate: bool = False,
                         five_view_resize=True):
    """The 8-bit frames of the reference's ``save_concatenated_videos`` / ``save_seperate_videos`` (video_utils.py:507-627),
    composed on the device: a generator of ``(i, frame)`` (``separate=False``: one merged frame per timestep, the keys' rows
    stacked in the order of ``keys``) or ``(key, i, frame)`` (``separate=True``: key by key, one row each), ``frame`` a host uint8
    array.  Per frame, each key's images ``[i * num_cams : (i + 1) * num_cams]`` lie side by side: colour lists as they are,
    ``gt_sky_masks`` on three channels, ``sky_masks`` as 1 - opacity, a key containing ``depth`` coloured by
    ``ops.compose_frame``'s depth rule with the opacity list named by replacing ``depths`` with ``opacities`` (``median_depths``
    falls back to ``opacities``).  A key that is absent or empty is skipped; a depth key without an opacity list is skipped in
    the merged mode and a ``KeyError`` in the separate one, as in the reference.  A merged frame that holds a depth row is
    scaled by 255 in fp64, every other frame in fp32 (numpy's promotion in the reference; they differ at rounding ties only).

    List entries are numpy arrays (uploaded frame by frame) or device tensors (``render(..., to_host=False)``).  ONE launch
    builds a frame; only its 3 bytes per pixel leave the GPU, into one of two alternating pinned buffers, while the next frame
    is composed.

    A group of exactly five images is what the reference's ``resize_five_views`` changes (utils/visualization_tools.py:36-49):
    views 0 and 4 become black with ``scipy.ndimage.zoom(img, [h / H, 1, 1])``, ``h = int(W * 0.46)``, clipped to [0, 1], in
    their bottom h rows.  ``five_view_resize="zoom"`` does that on the device (``ops.five_view_frame``: one more launch per
    frame, still 3 bytes per pixel leaving the GPU); a depth row's resized views are fp64 images there and are scaled by 255 in
    fp64 in the separate mode too; ``h > H`` (where the reference fails) and ``h < 2`` raise ``ValueError``.  The default,
    ``True``, keeps raising ``NotImplementedError`` for five views -- the zoom is asked for by name, as ``lo="auto"`` is -- and
    ``False`` tiles the five views UNRESIZED, which is not the reference's picture.

    Deviations from the reference: a NaN colour is written as 0 (numpy leaves that cast undefined); a non-finite value in a
    resized view spoils its own column and channel of that view (the reference: the whole view); images that are neither
    [H, W, 3] nor one of the single-channel cases, or whose sizes differ within a frame, raise ``ValueError``."""
    if five_view_resize not in (True, False, "zoom"):
        raise ValueError(f'five_view_resize is True, False or "zoom", not {five_view_resize!r}')
    plan = _frame_plan(render_results, keys, separate)
    if not plan:
        if separate:
            return
        raise ValueError(f"compose_video_frames: none of the keys {list(keys)} has images")
    device = None
    for _, _, images, opacities in plan:
        for x in list(images[:1]) + list((opacities or [])[:1]):
            if isinstance(x, Tensor) and x.is_cuda:
                device = x.device
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    pinned: Dict[int, Tensor] = {}
    n_frames = 0

    def start(rows):
        """Compose one frame of ``rows`` and start its transfer: (host view, event, the device frame)."""
        nonlocal n_frames
        tiles, H, W, cams = [], None, None, None
        for r, (key, kind, images, opacities) in enumerate(rows):
            if len(images) == 0 or (cams is not None and len(images) != cams):
                raise ValueError(f"{key}: {len(images)} images in a frame" + ("" if cams is None else f" whose other rows have {cams}"))
            cams = len(images)
            if opacities is not None and len(opacities) < cams:
                raise ValueError(f"{key}: {len(opacities)} opacity images for {cams} depth images")
            for c, x in enumerate(images):
                t = _tile_image(x, kind, key, device)
                o = None if opacities is None else _tile_image(opacities[c], "depth", key, device)
                if H is None:
                    H, W = int(t.shape[0]), int(t.shape[1])
                if tuple(t.shape[:2]) != (H, W) or (o is not None and tuple(o.shape) != (H, W)):
                    raise ValueError(f"{key}: an image of {tuple(t.shape[:2])} in a frame of {(H, W)} images")
                tiles.append((kind, r, c, t, o))
        if cams == 5 and five_view_resize and five_view_resize != "zoom":
            raise NotImplementedError("compose_video_frames: groups of five views are resized by the reference with a cubic-spline zoom "
                                      '(resize_five_views): pass five_view_resize="zoom" for it, or five_view_resize=False to tile them '
                                      "unresized")
        fp64 = (not separate) and any(kind == "depth" for _, kind, _, _ in rows)
        if cams == 5 and five_view_resize == "zoom":
            frame = ops.five_view_frame(tiles, H, W, len(rows), fp64)
        else:
            frame = ops.compose_frame(tiles, H, W, len(rows), cams, fp64)
        slot = n_frames & 1
        n_frames += 1
        buf = pinned.get(slot)
        if buf is None or buf.numel() < frame.numel():
            buf = pinned[slot] = torch.empty((frame.numel(),), dtype=torch.uint8, pin_memory=True)
        host = buf[:frame.numel()].view(frame.shape)
        host.copy_(frame, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev, frame

    def finish(item) -> np.ndarray:
        host, ev, _ = item
        ev.synchronize()
        return host.numpy().copy()      # the pinned buffer is reused two frames later

    def cut(lst, i):
        return lst[i * num_cams:(i + 1) * num_cams]

    with torch.no_grad(), torch.cuda.device(device):
        if separate:
            jobs = [((key, i), [(key, kind, cut(images, i), None if opacities is None else cut(opacities, i))])
                    for key, kind, images, opacities in plan for i in range(num_timestamps)]
        else:
            jobs = [((i,), [(key, kind, cut(images, i), None if opacities is None else cut(opacities, i)) for key, kind, images, opacities in plan])
                    for i in range(num_timestamps)]
        pending = None
        for tag, rows in jobs:
            item = (tag, start(rows))
            if pending is not None:     # frame i leaves while frame i + 1 is composed
                yield (*pending[0], finish(pending[1]))
            pending = item
        if pending is not None:
            yield (*pending[0], finish(pending[1]))


def _imageio():
    try:
        import imageio
    except ImportError as e:
        raise ImportError("save_videos writes through imageio, which is not installed; install it or pass writer_factory "
                          "(and image_writer for save_images)") from e
    return imageio


def save_videos(render_results: Dict[str, list], save_pth: str, num_timestamps: int, keys: List[str] = ["gt_rgbs", "rgbs", "depths"],
                num_cams: int = 3, save_seperate_video: bool = False, save_images: bool = False, fps: int = 10, verbose: bool = True,
                writer_factory=None, image_writer=None, five_view_resize=True):
    """video_utils.py:471-504 on ``compose_video_frames``: the reference's signature (spelling included) and return value.
    ``writer_factory(path, mode="I"[, fps=fps])`` returns an object with ``append_data(frame)`` and ``close()`` and
    ``image_writer(path, image)`` writes one image; by default they are ``imageio.get_writer`` / ``imageio.imwrite``, imported
    when first needed (``ImportError`` when imageio is absent).  ``five_view_resize``: see ``compose_video_frames``."""
    fn = save_seperate_videos if save_seperate_video else save_concatenated_videos
    return fn(render_results, save_pth, num_timestamps=num_timestamps, keys=keys, num_cams=num_cams, save_images=save_images, fps=fps,
              verbose=verbose, writer_factory=writer_factory, image_writer=image_writer, five_view_resize=five_view_resize)


def _open_writer(writer_factory, path: str, num_timestamps: int, fps: int):
    factory = writer_factory if writer_factory is not None else _imageio().get_writer
    return factory(path, mode="I") if num_timestamps == 1 else factory(path, mode="I", fps=fps)   # one timestep: it's an image


def save_concatenated_videos(render_results: Dict[str, list], save_pth: str, num_timestamps: int,
                             keys: List[str] = ["gt_rgbs", "rgbs", "depths"], num_cams: int = 3, save_images: bool = False, fps: int = 10,
                             verbose: bool = True, writer_factory=None, image_writer=None, five_view_resize=True):
    """video_utils.py:507-565: one merged frame per timestep to one writer; returns ``{"concatenated_frame": frame}`` with the
    frame at ``num_timestamps // 2`` (frame 0 of a single timestep).  ``save_images`` is ignored here, as in the reference."""
    return_frame_id = 0 if num_timestamps == 1 else num_timestamps // 2
    writer = _open_writer(writer_factory, save_pth, num_timestamps, fps)
    return_frame = None
    for i, frame in compose_video_frames(render_results, num_timestamps, keys, num_cams, False, five_view_resize):
        if i == return_frame_id:
            return_frame = frame
        writer.append_data(frame)
    writer.close()
    if verbose:
        logger.info(f"saved video to {save_pth}")
    return {"concatenated_frame": return_frame}


def save_seperate_videos(render_results: Dict[str, list], save_pth: str, num_timestamps: int,
                         keys: List[str] = ["gt_rgbs", "rgbs", "depths"], num_cams: int = 3, fps: int = 10, verbose: bool = False,
                         save_images: bool = False, writer_factory=None, image_writer=None, five_view_resize=True):
    """video_utils.py:568-627: one video per key at ``<save_pth>_<key>.mp4`` (or ``.png``); returns ``{key: frame}`` with each
    key's frame at ``num_timestamps // 2``.  ``save_images`` also writes every view of every frame to
    ``<save_pth>_<key>_<i * 3 + j>.png`` -- the reference's numbering, whatever ``num_cams`` is.  One deviation: no writer is
    opened for a key that is then skipped (the reference opens one and leaves it)."""
    import os
    return_frame_id = num_timestamps // 2
    return_frame_dict, writer, current, path = {}, None, None, None
    for key, i, frame in compose_video_frames(render_results, num_timestamps, keys, num_cams, True, five_view_resize):
        if key != current:
            if writer is not None:
                writer.close()
                if verbose:
                    logger.info(f"saved video to {path}")
            path = save_pth.replace(".mp4", f"_{key}.mp4").replace(".png", f"_{key}.png")
            writer, current = _open_writer(writer_factory, path, num_timestamps, fps), key
        if save_images:
            write = image_writer if image_writer is not None else _imageio().imwrite
            if i == 0:
                os.makedirs(path.replace(".mp4", ""), exist_ok=True)
            n = len(render_results["opacities" if key == "sky_masks" else key][i * num_cams:(i + 1) * num_cams])
            W = frame.shape[1] // n
            for j in range(n):      # a view's 8-bit image is its columns of the row: every tile is cut to 8 bits on its own
                write(path.replace(".mp4", f"_{i*3 + j:03d}.png"), np.ascontiguousarray(frame[:, j * W:(j + 1) * W]))
        writer.append_data(frame)
        if i == return_frame_id:
            return_frame_dict[key] = frame
    if writer is not None:
        writer.close()
        if verbose:
            logger.info(f"saved video to {path}")
    return return_frame_dict


def _non_zero_mean(x: List[float]) -> float:
    """video_utils.py:45-47."""
    return sum(x) / len(x) if len(x) > 0 else -1


def _psnr(sq_sum: float, n: float) -> float:
    """datasets/metrics.py:31-46 from a squared-error sum over n entries."""
    return float(-10.0 * np.log10(sq_sum / n))
