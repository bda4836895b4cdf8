"""The lifted feature field: utils/visualization_tools.py:visualize_voxels (:456-701) up to, and not including, its plotly
figure.  Rendered depths become occupied voxels, the voxels are filtered by queried density and coloured by the PCA of the
feature head -- with the grids held as bit masks and marked, compacted and gathered by the kernels of csrc/voxels.hip."""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Union

import torch
from torch import Tensor

from . import ops
from .render_utils import render_rays
from .video_utils import get_robust_pca

STATIC_MAX_DEPTH = 80.0          # :549
STATIC_DENSITY_THRESHOLD = 0.5   # :637
DYNAMIC_DENSITY_THRESHOLD = 0.1  # :677
DYNAMIC_RES_FACTOR = 0.8         # :490
QUERY_CHUNK = 2 ** 18            # :613
DYNAMIC_QUERY_STRIDE = 10        # :662


def vis_aabb(model_aabb) -> Tensor:
    """The box of the visualisation as a flat fp32 CPU tensor of 6 (:475-478): the model's box with the flattened elements
    ``[1:3] -= 1`` and ``[3:] += 1`` -- the reference's slice, so y_min, z_min and the three maxima move and x_min does not."""
    a = torch.as_tensor(model_aabb, dtype=torch.float32).detach().cpu().reshape(-1).clone()
    if a.numel() != 6:
        raise ops._lib.EmerError(f"vis_aabb: an aabb has 6 elements, got {a.numel()}")
    a[1:3] -= 1
    a[3:] += 1
    return a


class VoxelGrid:
    """An occupancy grid over ``aabb`` (6 values: min, max) as a bit mask on ``device``.  ``voxel_size_or_res``: a voxel edge
    length, giving ``res = ceil((max - min) / size)`` (:483-485, in fp32 on the host), or the resolution itself (3 ints).  The
    voxel size the kernels divide by is ``(max - min) / res`` in fp32 (datasets/utils.py:85)."""

    def __init__(self, aabb, voxel_size_or_res: Union[float, Sequence[int]], device) -> None:
        a = torch.as_tensor(aabb, dtype=torch.float32).detach().cpu().reshape(-1)
        if a.numel() != 6:
            raise ops._lib.EmerError(f"VoxelGrid: an aabb has 6 elements, got {a.numel()}")
        self.aabb_min, self.aabb_max = a[:3].clone(), a[3:].clone()
        if isinstance(voxel_size_or_res, (int, float)):
            res = torch.ceil((self.aabb_max - self.aabb_min) / voxel_size_or_res).long()
        else:
            res = torch.as_tensor(voxel_size_or_res).detach().cpu().reshape(-1).long()
        self.res = tuple(int(r) for r in res)
        self.voxel_size = (self.aabb_max - self.aabb_min) / res
        self.n_voxels = ops._voxel_count(self.res, "VoxelGrid")
        self.device = torch.device(device)
        self.bits = torch.zeros(ops.bit_words(self.n_voxels), dtype=torch.int32, device=self.device)
        self._min, self._size = tuple(self.aabb_min.tolist()), tuple(self.voxel_size.tolist())

    def job(self, origins: Tensor, viewdirs: Tensor, depth: Tensor, max_depth: float = math.inf):
        """This grid's member of an ``ops.voxel_mark`` launch."""
        return (origins, viewdirs, depth, max_depth, self._min, self._size, self.res, self.bits)

    def mark(self, origins: Tensor, viewdirs: Tensor, depth: Tensor, max_depth: float = math.inf) -> None:
        """Set the voxels that hold ``origins + viewdirs * depth`` for the rays with ``depth < max_depth``."""
        ops.voxel_mark([self.job(origins, viewdirs, depth, max_depth)])

    def occupied_points(self, want_indices: bool = False):
        """World corners of the set voxels in row-major order ([M, 3] fp32; with ``want_indices`` also [M, 3] int32 indices)."""
        return ops.bits_nonzero_voxels(self.bits, self.res, self._min, self._size, want_indices)

    def clear(self) -> None:
        self.bits.zero_()


def _default_render_func(cfg, model, proposal_estimator, proposal_networks) -> Callable:
    def render_func(data_dict: Dict[str, Tensor], lidar: bool) -> Dict[str, Tensor]:
        if lidar:   # forced lidar mode: the renderer skips colours and features (:525-540)
            return render_rays(radiance_field=model, proposal_estimator=proposal_estimator, proposal_networks=proposal_networks,
                               data_dict=data_dict, cfg=cfg, proposal_requires_grad=False, prefix="lidar_", return_decomposition=True)
        return render_rays(radiance_field=model, proposal_estimator=proposal_estimator, proposal_networks=proposal_networks,
                           data_dict=data_dict, cfg=cfg, proposal_requires_grad=False)
    return render_func


def _colours(feats: Optional[Tensor], pca) -> Optional[Tensor]:
    return None if feats is None else ops.feature_colours(feats, *pca)


def lift_voxels(cfg, model, proposal_estimator=None, proposal_networks=None, dataset=None, is_dynamic: bool = False, pca=None,
                render_func: Optional[Callable] = None) -> dict:
    """``visualize_voxels`` without the figure: ``{"coords", "colors", "dynamic_coords", "dynamic_colors", "vis_aabb", "pca"}``,
    the static entries device tensors ([M, 3]), the dynamic ones lists of device tensors (None when not ``is_dynamic``),
    ``vis_aabb`` a list of 6 floats and ``pca`` the (matrix, min, max) that coloured the points.  Reads ``cfg.render.vis_voxel_size``
    and what ``render_rays`` reads; ``dataset`` gives ``full_pixel_set``, ``num_cams`` and
    ``pixel_source.unique_normalized_timestamps``.  ``pca``: a (matrix [E, 3], min [3], max [3]) to use instead of
    ``get_robust_pca(patches, m=2.5)`` of the first ``num_cams`` images.  ``render_func(data_dict, lidar)`` replaces the two
    ``render_rays`` calls (full render for the PCA patches; forced-lidar render with decomposition for the depths).  A model
    without the feature head gives ``colors=None`` (the reference raises).  The reference's quirks are kept, see the comments."""
    if proposal_networks is None:
        raise ops._lib.EmerError("lift_voxels: proposal_networks is required")
    modules = [model, *proposal_networks] + ([proposal_estimator] if proposal_estimator is not None else [])
    modes = [m.training for m in modules]
    for m in modules:
        m.eval()
    try:
        with torch.no_grad():
            return _lift_voxels(cfg, model, proposal_estimator, proposal_networks, dataset, is_dynamic, pca, render_func)
    finally:
        for m, training in zip(modules, modes):
            m.train(training)


def _lift_voxels(cfg, model, proposal_estimator, proposal_networks, dataset, is_dynamic, pca, render_func) -> dict:
    device = model.device
    if render_func is None:
        render_func = _default_render_func(cfg, model, proposal_estimator, proposal_networks)
    has_feats = bool(getattr(model, "enable_feature_head", False))
    box = vis_aabb(model.aabb)
    size = cfg.render.vis_voxel_size
    static_grid = VoxelGrid(box, size, device)
    dynamic_grid, dynamic_candidates = None, []
    if is_dynamic:   # a slightly smaller voxel count for the dynamic voxels (:489-491)
        dynamic_grid = VoxelGrid(box, torch.ceil((box[3:] - box[:3]) / size * DYNAMIC_RES_FACTOR).long(), device)
    patches: List[Tensor] = []
    pixel_set = dataset.full_pixel_set
    for i in range(len(pixel_set)):
        data_dict = {k: v.to(device) for k, v in pixel_set[i].items()}
        if i < dataset.num_cams:
            # the first timestep is also rendered in full, for the PCA patches (:508-524)
            full = render_func(data_dict, False)
            if has_feats:
                feats = full["dino_pe_free"] if "dino_pe_free" in full else full["dino_feat"]
                patches.append(feats.reshape(-1, feats.shape[-1]))
        data_dict["lidar_origins"] = data_dict["origins"]
        data_dict["lidar_viewdirs"] = data_dict["viewdirs"]
        data_dict["lidar_normed_timestamps"] = data_dict["normed_timestamps"]
        res = render_func(data_dict, True)
        o, d = data_dict["lidar_origins"], data_dict["lidar_viewdirs"]
        jobs = [static_grid.job(o, d, res["static_depth"] if is_dynamic else res["depth"], STATIC_MAX_DEPTH)]
        if is_dynamic:
            jobs.append(dynamic_grid.job(o, d, res["dynamic_depth"]))      # no depth filter (:571-592)
        ops.voxel_mark(jobs)
        # the reference's grouping (:593): num_cams + 1 images in the first group, the tail is dropped
        if is_dynamic and i % dataset.num_cams == 0 and i > 0:
            dynamic_candidates.append(dynamic_grid.occupied_points())
            dynamic_grid.clear()
    if has_feats and pca is None:
        pca = get_robust_pca(torch.cat(patches, dim=0), m=2.5)
    if pca is not None:
        pca = tuple(p.to(device) for p in pca)

    # static voxels: the mean density over every proposal network and the model decides (:621-638)
    candidates = static_grid.occupied_points()
    points, colours = [], []
    for s in range(0, candidates.shape[0], QUERY_CHUNK):
        chunk = candidates[s:s + QUERY_CHUNK]
        densities = [p(chunk)["density"].squeeze(-1) for p in proposal_networks]
        densities.append(model.forward(chunk, query_feature_head=False)["density"].reshape(-1))
        kept = ops.bits_select_rows(ops.mean_threshold_bits(densities, STATIC_DENSITY_THRESHOLD), chunk)
        if kept.shape[0] == 0:
            continue
        points.append(kept)
        if has_feats:
            colours.append(_colours(model.forward(kept, query_feature_head=True, query_pe_head=False)["dino_feat"], pca))
    coords = torch.cat(points, dim=0) if points else torch.empty(0, 3, device=device)
    colors = (torch.cat(colours, dim=0) if colours else torch.empty(0, 3, device=device)) if has_feats else None

    dynamic_coords = dynamic_colors = None
    if is_dynamic:
        dynamic_coords, dynamic_colors = [], []
        unq = dataset.pixel_source.unique_normalized_timestamps.to(device)
        for g in range(0, len(dynamic_candidates), DYNAMIC_QUERY_STRIDE):      # every 10th group, at timestamp g (:662-696)
            chunk = dynamic_candidates[g]
            if chunk.shape[0] == 0:
                continue
            ts = unq[g].repeat(chunk.shape[0], 1)
            density = model.forward(chunk, data_dict={"normed_timestamps": ts}, query_feature_head=False)["dynamic_density"]
            kept = ops.bits_select_rows(ops.mean_threshold_bits([density.reshape(-1)], DYNAMIC_DENSITY_THRESHOLD), chunk)
            if kept.shape[0] == 0:
                continue
            dynamic_coords.append(kept)
            if has_feats:
                ts = unq[g].repeat(kept.shape[0], 1)
                feats = model.forward(kept, data_dict={"normed_timestamps": ts}, query_feature_head=True, query_pe_head=False)
                dynamic_colors.append(_colours(feats["dynamic_dino_feat"], pca))
        if not has_feats:
            dynamic_colors = None
    return {"coords": coords, "colors": colors, "dynamic_coords": dynamic_coords, "dynamic_colors": dynamic_colors,
            "vis_aabb": box.tolist(), "pca": pca}
