"""Plain torch restatement, on CPU tensors, of the stages of the voxel lift (the reference's utils/visualization_tools.py:456-701
and datasets/utils.py:47-52,85-88): ray end points -> set of linear voxel indices, nonzero order, world corners, the
mean-threshold selector and the row gather.  Every stage is the reference's fp32 expression in the reference's order, with the
two rules the kernels add where the reference is undefined: the range test is made on the float quotient, and a row with a
non-finite coordinate is dropped."""
from __future__ import annotations

import math

import torch

CHUNK = 2 ** 18


def vis_aabb(model_aabb) -> torch.Tensor:
    """:475-478: the model's box, flattened, elements [1:3] lowered and [3:] raised by one (x_min is not expanded)."""
    a = torch.as_tensor(model_aabb, dtype=torch.float32).detach().cpu().reshape(-1).clone()
    a[1:3] -= 1
    a[3:] += 1
    return a


def resolution(aabb: torch.Tensor, voxel_size: float, factor=None):
    """:483-485 / :489-491: ceil((max - min) / size [* 0.8]) in fp32."""
    q = (aabb[3:] - aabb[:3]) / voxel_size
    if factor is not None:
        q = q * factor
    return tuple(int(v) for v in torch.ceil(q).long())


def voxel_size(aabb: torch.Tensor, res) -> torch.Tensor:
    """datasets/utils.py:85: (aabb_max - aabb_min) / res, fp32 over int64."""
    return (aabb[3:] - aabb[:3]) / torch.tensor(res, dtype=torch.int64)


def mark(origins, viewdirs, depth, aabb, res, max_depth=math.inf) -> torch.Tensor:
    """The sorted, unique linear indices (ix * ry + iy) * rz + iz of the voxels that one image marks."""
    o, d = origins.reshape(-1, 3).float(), viewdirs.reshape(-1, 3).float()
    t = depth.reshape(-1, 1).float()
    world = o + d * t
    world = world[t.squeeze(-1) < max_depth]
    v = (world - aabb[:3]) / voxel_size(aabb, res)
    r = torch.tensor(res, dtype=torch.float32)
    keep = ((v > -1.0) & (v < r)).all(-1)              # trunc(v) in [0, res) <=> -1 < v < res; NaN fails
    i = v[keep].long()                                 # truncates toward zero
    lin = (i[:, 0] * res[1] + i[:, 1]) * res[2] + i[:, 2]
    return torch.unique(lin)                           # sorted


def indices_of(lin: torch.Tensor, res) -> torch.Tensor:
    """Linear indices -> [M, 3] (ix, iy, iz), the rows of torch.nonzero of the grid."""
    iz = lin % res[2]
    iy = (lin // res[2]) % res[1]
    ix = lin // (res[1] * res[2])
    return torch.stack([ix, iy, iz], -1)


def world_corners(lin: torch.Tensor, aabb, res) -> torch.Tensor:
    """voxel_coords_to_world_coords: aabb_min + points * voxel_size with int64 points."""
    return aabb[:3] + indices_of(lin, res) * voxel_size(aabb, res)


def mean_selector(densities, thr: float) -> torch.Tensor:
    """mean(stack(densities), 0) > thr with THE rule of the kernels: a sequential fp32 sum, then one division by K."""
    s = densities[0].reshape(-1).float().clone()
    for d in densities[1:]:
        s = s + d.reshape(-1).float()
    return (s / float(len(densities))) > thr


def select_rows(selector: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    return src[selector]


def bits_of(selector: torch.Tensor) -> torch.Tensor:
    """A boolean vector as the int32 words of its bit mask (bit n: word n // 32, position n % 32)."""
    n = selector.numel()
    pad = torch.zeros((n + 31) // 32 * 32, dtype=torch.int64)
    pad[:n] = selector.reshape(-1).long()
    w = (pad.reshape(-1, 32) << torch.arange(32)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def colours(feat, mat, lo, hi) -> torch.Tensor:
    """:648-651, in fp32 as the reference evaluates them: feats @ M, (c - min) / (max - min), clamp."""
    c = feat.float() @ mat.float()
    return torch.clamp((c - lo.float()) / (hi.float() - lo.float()), 0, 1)


def groups(n_images: int, num_cams: int):
    """The reference's grouping of the dynamic grid (:593): it is read out and cleared after image i when i % num_cams == 0 and
    i > 0, so the first group holds num_cams + 1 images and the tail is dropped."""
    out, start = [], 0
    for i in range(n_images):
        if i % num_cams == 0 and i > 0:
            out.append(list(range(start, i + 1)))
            start = i + 1
    return out


def lift(rendered, aabb, vis_voxel_size: float, num_cams: int, is_dynamic: bool):
    """Candidate voxels of the whole loop from what was rendered per image (``rendered``: list of dicts with CPU ``origins``,
    ``viewdirs``, ``depth``, ``static_depth``, ``dynamic_depth``): (static linear indices, [dynamic linear indices per group])."""
    res = resolution(aabb, vis_voxel_size)
    static = torch.unique(torch.cat([mark(r["origins"], r["viewdirs"], r["static_depth" if is_dynamic else "depth"], aabb, res, 80.0)
                                     for r in rendered]))
    dyn = []
    if is_dynamic:
        dres = resolution(aabb, vis_voxel_size, 0.8)
        for g in groups(len(rendered), num_cams):
            dyn.append(torch.unique(torch.cat([mark(rendered[i]["origins"], rendered[i]["viewdirs"], rendered[i]["dynamic_depth"], aabb, dres)
                                               for i in g])))
    return static, dyn


def face_allowance(rendered, key, tols, aabb, res, max_depth=math.inf, slack=1e-4) -> torch.Tensor:
    """The voxels whose occupancy a change of the rendered depths within ``tols`` (per image: per-ray bounds on ``rendered[i][key]``)
    can alter, as sorted linear indices.  In float64: a ray is unstable when its end points at depth - tol, depth and depth + tol
    do not share one voxel (``slack`` metres are added to tol for the fp32 rounding of the chain itself), or when its depth lies
    within tol of ``max_depth``; an unstable ray flags every in-range voxel of the box spanned by those end points."""
    vs, amin = voxel_size(aabb, res).double(), aabb[:3].double()
    r3 = torch.tensor(res, dtype=torch.float64)
    out = [torch.empty(0, dtype=torch.int64)]
    for r, tol in zip(rendered, tols):
        o, d = r["origins"].reshape(-1, 3).double(), r["viewdirs"].reshape(-1, 3).double()
        t = r[key].reshape(-1).double()
        tol = tol.reshape(-1).double() + slack
        idx = [torch.trunc((o + d * (t + s * tol)[:, None] - amin) / vs) for s in (-1, 0, 1)]
        lo, hi = torch.stack(idx).min(0).values, torch.stack(idx).max(0).values
        unstable = ((lo != hi).any(-1) | ((t - max_depth).abs() <= tol)) & (t < max_depth + tol)
        lo, hi = lo[unstable], hi[unstable]
        for corner in range(8):
            i = torch.stack([hi[:, c] if (corner >> c) & 1 else lo[:, c] for c in range(3)], -1)
            i = i[((i >= 0) & (i < r3)).all(-1)].long()
            out.append((i[:, 0] * res[1] + i[:, 1]) * res[2] + i[:, 2])
    return torch.unique(torch.cat(out))
