"""Training / rendering ray source on device-resident dataset tensors.

Mirrors the ray-facing part of the reference's ``ScenePixelSource`` (datasets/base/pixel_source.py): ``get_rays``
(:39-76), ``sample_uniform_rays`` (:622-668), ``sample_important_rays`` (:564-620), ``get_train_rays`` (:670-731),
``get_render_rays`` (:733-846, at any ``downscale_factor``, :955-976), ``build_pixel_error_buffer`` /
``update_pixel_error_maps`` (:462-517) and its on-device form ``accumulate_pixel_error`` / ``finish_pixel_error_maps``.
Loading images / poses from disk (the dataset classes proper) stays out of scope: the constructor takes the tensors the
reference's loaders produce.

Every per-batch operation is a HIP kernel (csrc/rays.hip): one launch for uniform pixels, a radix-select race for the
error-buffer multinomial (no host round trip), one gather kernel for rays + colours + masks + timestamps, and (when the
source has them) one more for the dynamic masks and the DINO feature rows (``get_features``, :439-468); a low-resolution
render image (antialiased bicubic colours, nearest masks, rays of the scaled camera, features) is one launch.  Random numbers
come from a counter-based generator keyed by a seed word in device memory (``self.seed_word``), advanced by one tiny
device op per batch, so a captured hipGraph replays with fresh rays.
"""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .ops import _check_cuda, _ptr, _stream

_SALT_UNIFORM, _SALT_RACE, _SALT_CELL = 0x1111, 0x2222, 0x3333


def get_rays(x: Tensor, y: Tensor, c2w: Tensor, intrinsic: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """pixel_source.py:39-76 for per-ray camera matrices: x, y [n] (any integer / float dtype), c2w [n,4,4] or [4,4],
    intrinsic [n,3,3] or [3,3] -> (origins [n,3], viewdirs [n,3], direction_norm [n,1])."""
    _check_cuda(x, y, c2w, intrinsic)
    n = x.numel()
    dev = x.device
    c2w = c2w.reshape(-1, 4, 4).float().contiguous()
    K = intrinsic.reshape(-1, 3, 3).float().contiguous()
    if c2w.shape[0] == 1 and K.shape[0] == 1:
        idx = torch.zeros(n, device=dev, dtype=torch.int64)
    else:
        assert c2w.shape[0] == n and K.shape[0] == n, "one camera per ray (or a single camera for all rays)"
        idx = torch.arange(n, device=dev, dtype=torch.int64)
    xi, yi = x.reshape(-1).to(torch.int64).contiguous(), y.reshape(-1).to(torch.int64).contiguous()
    o, d = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
    nrm = torch.empty((n, 1), device=dev)
    with torch.cuda.device(dev):
        _lib.call("emer_gen_rays", _ptr(idx), _ptr(yi), _ptr(xi), _ptr(c2w), _ptr(K), None, None, None, None, n, 1, 1, _ptr(o), _ptr(d),
                  _ptr(nrm), None, None, None, None, None, _stream(o))
    return o, d, nrm


def _cubic(x: np.ndarray, a: float = -0.5) -> np.ndarray:
    """Keys' cubic convolution kernel (a = -0.5: torch's antialiased bicubic filter)."""
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def antialias_bicubic_tables(in_size: int, out_size: int, scale_factor: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """One axis of torch's ``interpolate(scale_factor=s, mode="bicubic", antialias=True)`` for s <= 1 as tables: output i sums
    the inputs xmin[i] .. xmin[i] + xsize[i] - 1 with the weights w[i, :xsize[i]] (zero beyond).  Support 2 / s, centre
    (i + 0.5) / s, window [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), in_size)), tap weight
    cubic((j - c + 0.5) * s) normalised over the window actually used (so image borders renormalise).  Computed in double
    precision and rounded to float32 once: a weight the kernel reads carries a single rounding."""
    inv = 1.0 / scale_factor
    support = 2.0 * inv
    k = int(math.ceil(support)) * 2 + 1
    centre = (np.arange(out_size, dtype=np.float64) + 0.5) * inv
    xmin = np.maximum((centre - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((centre + support + 0.5).astype(np.int64), in_size)
    xsize = xmax - xmin
    j = np.arange(k, dtype=np.int64)[None, :]
    w = _cubic((j + xmin[:, None] - centre[:, None] + 0.5) * scale_factor)
    w = np.where(j < xsize[:, None], w, 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    assert xsize.min() >= 1 and xsize.max() <= k and xmin.min() >= 0 and (xmin + xsize).max() <= in_size
    return xmin.astype(np.int32), xsize.astype(np.int32), w.astype(np.float32)


class PixelSource:
    """images [n_imgs,H,W,3] fp32 in [0,1], cam_to_worlds [n_imgs,4,4], intrinsics [n_imgs,3,3] (all on the GPU);
    optional sky_masks [n_imgs,H,W], normalized_timestamps [n_imgs], cam_ids [n_imgs]; keyword-only dynamic_masks
    [n_imgs,H,W] (any dtype, stored as float like the reference's loader, :256-268) and features [n_imgs,Hf,Wf,E] (DINO
    feature maps, stored fp32 on the device).  A feature row is looked up at ((y * Hf / H).long(), (x * Wf / W).long()) in
    torch's float32 arithmetic (``featmap_downscale_factor``, :318-321)."""

    def __init__(self, images: Tensor, cam_to_worlds: Tensor, intrinsics: Tensor, sky_masks: Optional[Tensor] = None,
                 normalized_timestamps: Optional[Tensor] = None, cam_ids: Optional[Tensor] = None, buffer_ratio: float = 0.0,
                 buffer_downscale: int = 4, seed: int = 0, *, dynamic_masks: Optional[Tensor] = None,
                 features: Optional[Tensor] = None) -> None:
        _check_cuda(images, cam_to_worlds, intrinsics, sky_masks, normalized_timestamps, cam_ids, dynamic_masks, features)
        self.images = images.float().contiguous()
        self.num_imgs, self.HEIGHT, self.WIDTH = self.images.shape[:3]
        self.cam_to_worlds = cam_to_worlds.float().contiguous()
        self.intrinsics = intrinsics.float().contiguous()
        self.sky_masks = None if sky_masks is None else sky_masks.float().contiguous()
        self.normalized_timestamps = None if normalized_timestamps is None else normalized_timestamps.float().contiguous()
        self.cam_ids = None if cam_ids is None else cam_ids.to(torch.int64).contiguous()
        self.dynamic_masks = None if dynamic_masks is None else dynamic_masks.float().contiguous()
        if self.dynamic_masks is not None and tuple(self.dynamic_masks.shape) != (self.num_imgs, self.HEIGHT, self.WIDTH):
            raise ValueError(f"dynamic_masks: expected {(self.num_imgs, self.HEIGHT, self.WIDTH)}, got {tuple(self.dynamic_masks.shape)}")
        self.features = None if features is None else features.float().contiguous()
        self.featmap_downscale_factor = None
        if self.features is not None:
            if self.features.dim() != 4 or self.features.shape[0] != self.num_imgs:
                raise ValueError(f"features: expected [{self.num_imgs}, Hf, Wf, E], got {tuple(self.features.shape)}")
            self.featmap_downscale_factor = (self.features.shape[1] / self.HEIGHT, self.features.shape[2] / self.WIDTH)
        self.device = self.images.device
        self.buffer_ratio, self.buffer_downscale = float(buffer_ratio), int(buffer_downscale)
        self.pixel_error_maps: Optional[Tensor] = None
        self.pixel_error_buffered = False
        self.seed_word = torch.tensor([seed], dtype=torch.int64, device=self.device)  # read by the kernels as uint64
        self._ws = torch.empty(4 + 2048, dtype=torch.int32, device=self.device)
        self._all = None
        self._downscale_factor = self._old_downscale_factor = 1.0
        self._resample_tables = None                  # (factor, device tables) of the low-resolution render path
        self._error_extrema: Optional[Tensor] = None  # [n_imgs, 2] per-image (min, max) of the error-buffer refresh
        self._error_rows_written: set = set()

    # ---------------------------------------------------------------------------------- downscale factor (:955-976)
    @property
    def downscale_factor(self) -> float:
        """Factor of ``get_render_rays`` (1.0: full resolution).  ``get_train_rays`` does not look at it (nor does the reference's)."""
        return self._downscale_factor

    def update_downscale_factor(self, downscale: float) -> None:
        self._old_downscale_factor = self._downscale_factor
        self._downscale_factor = downscale

    def reset_downscale_factor(self) -> None:
        """Back to the value before the last ``update_downscale_factor``."""
        self._downscale_factor = self._old_downscale_factor

    # ------------------------------------------------------------------------------------ error buffer (:462-517)
    def build_pixel_error_buffer(self) -> None:
        if self.buffer_ratio > 0:
            self.pixel_error_maps = torch.ones((self.num_imgs, self.HEIGHT // self.buffer_downscale, self.WIDTH // self.buffer_downscale),
                                               dtype=torch.float32, device=self.device)

    def update_pixel_error_maps(self, pred_rgbs: Tensor, gt_rgbs: Tensor, dynamic_opacities: Optional[Tensor] = None) -> None:
        """|gt - pred| averaged over colour at the buffer's resolution, x5 where the dynamic opacity exceeds 0.1,
        normalised to [0, 1] (offline: runs once per evaluation, plain torch)."""
        if self.pixel_error_maps is None:
            return
        err = (gt_rgbs.to(self.device) - pred_rgbs.to(self.device)).abs().mean(dim=-1)
        assert err.shape == self.pixel_error_maps.shape
        if dynamic_opacities is not None:
            err = torch.where(dynamic_opacities.to(self.device).reshape(err.shape) > 0.1, err * 5, err)
        self.pixel_error_maps = ((err - err.min()) / (err.max() - err.min())).contiguous()
        self.pixel_error_buffered = True

    def accumulate_pixel_error(self, img_idx: int, pred_rgb: Tensor, gt_rgb: Tensor, dynamic_opacity: Optional[Tensor] = None) -> None:
        """One image's share of ``update_pixel_error_maps`` on the device: mean_c |gt - pred| (x5 where the dynamic opacity
        exceeds 0.1) written INTO the buffer's row ``img_idx`` -- the buffer keeps its storage, so a captured sampler graph
        keeps reading it -- and the row's (min, max) left in a small device array for ``finish_pixel_error_maps``.  pred_rgb /
        gt_rgb: [Hb, Wb, 3] (or [Hb * Wb, 3]) fp32 on the device at the buffer's resolution; one launch, no host transfer.
        Between the first call of a refresh and ``finish_pixel_error_maps`` the buffer holds unnormalised rows."""
        if self.pixel_error_maps is None:
            return
        _check_cuda(pred_rgb, gt_rgb, dynamic_opacity)
        maps = self.pixel_error_maps
        cells = maps.shape[1] * maps.shape[2]
        if not 0 <= int(img_idx) < self.num_imgs:
            raise IndexError(f"accumulate_pixel_error: image {img_idx} of {self.num_imgs}")
        if pred_rgb.numel() != cells * 3 or gt_rgb.numel() != cells * 3 or (dynamic_opacity is not None and dynamic_opacity.numel() != cells):
            raise ValueError(f"accumulate_pixel_error: expected {tuple(maps.shape[1:])} x 3 colours (and as many opacities), got "
                             f"{tuple(pred_rgb.shape)}, {tuple(gt_rgb.shape)}" + ("" if dynamic_opacity is None else f", {tuple(dynamic_opacity.shape)}"))
        assert maps.is_contiguous() and maps.dtype == torch.float32
        pred, gt = pred_rgb.detach().float().contiguous(), gt_rgb.detach().float().contiguous()
        opa = None if dynamic_opacity is None else dynamic_opacity.detach().float().contiguous()
        if self._error_extrema is None:
            self._error_extrema = torch.empty((self.num_imgs, 2), dtype=torch.float32, device=self.device)
        row, ext = maps[int(img_idx)], self._error_extrema[int(img_idx)]
        with torch.cuda.device(self.device):
            _lib.call("emer_pixel_error_image", _ptr(pred), _ptr(gt), _ptr(opa), cells, _ptr(row), _ptr(ext), _stream(maps))
        self._error_rows_written.add(int(img_idx))
        self._support_cache = None    # a raw-pointer write does not bump the tensor's version counter

    def finish_pixel_error_maps(self) -> None:
        """Normalise the whole buffer to (e - min) / (max - min) in place, in one launch that also reduces the per-image
        extrema.  Every image must have been given to ``accumulate_pixel_error`` since the last finish (the reference
        normalises over the full set too).  max == min gives NaN in every cell, as the reference's division does."""
        if self.pixel_error_maps is None:
            return
        missing = set(range(self.num_imgs)) - self._error_rows_written
        if missing:
            raise RuntimeError(f"finish_pixel_error_maps: {len(missing)} of {self.num_imgs} images were not accumulated (first: {min(missing)})")
        maps = self.pixel_error_maps
        with torch.cuda.device(self.device):
            _lib.call("emer_pixel_error_normalise", _ptr(maps), maps.numel(), _ptr(self._error_extrema), self.num_imgs, _stream(maps))
        self._error_rows_written = set()
        self._support_cache = None
        self.pixel_error_buffered = True

    # ------------------------------------------------------------------------------------------------ sampling
    def _candidates(self, cand) -> Tuple[Optional[Tensor], int]:
        if cand is None:
            return None, self.num_imgs
        if not isinstance(cand, Tensor):
            cand = torch.tensor(cand)
        cand = cand.to(self.device, torch.int64).contiguous()
        return cand, cand.numel()

    def _next_seed(self) -> None:
        self.seed_word.add_(0x9E3779B9)  # device-side: graph-capturable

    def sample_uniform_rays(self, num_rays: int, img_candidate_indices=None, advance: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """:622-668 -> (img_id, y, x), int64 [num_rays].  Every call draws fresh pixels (the seed word advances on the device;
        ``advance=False``: the caller advances it once for a group of draws, as get_train_rays does)."""
        cand, n_c = self._candidates(img_candidate_indices)
        img, y, x = (torch.empty(num_rays, dtype=torch.int64, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            _lib.call("emer_sample_uniform", _ptr(self.seed_word), _SALT_UNIFORM, num_rays, _ptr(cand), n_c, self.HEIGHT, self.WIDTH,
                      _ptr(img), _ptr(y), _ptr(x), _stream(img))
        if advance:
            self._next_seed()
        return img, y, x

    def sample_important_rays(self, num_rays: int, img_candidate_indices=None, advance: bool = True,
                              check_support: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
        """:564-620: multinomial over the error buffer of the candidate images WITHOUT replacement, then a random pixel of
        the chosen buffer cell.  Like torch.multinomial, asking for more samples than there are cells of positive weight is
        an error (``check_support``: one device->host read; a captured graph passes False after checking once)."""
        assert self.pixel_error_buffered, "Pixel error buffer not built."
        cand, n_c = self._candidates(img_candidate_indices)
        maps = self.pixel_error_maps if cand is None else self.pixel_error_maps[cand].contiguous()
        if check_support:
            n_pos = int((maps > 0).sum())
            if num_rays > n_pos:
                raise RuntimeError(f"sample_important_rays: cannot draw {num_rays} cells without replacement from {n_pos} cells of positive weight")
        Hb, Wb = maps.shape[1:]
        flat = torch.empty(num_rays, dtype=torch.int64, device=self.device)
        img, y, x = (torch.empty(num_rays, dtype=torch.int64, device=self.device) for _ in range(3))
        with torch.cuda.device(self.device):
            st = _stream(flat)
            _lib.call("emer_sample_importance", _ptr(maps), maps.numel(), _ptr(self.seed_word), _SALT_RACE, num_rays, _ptr(self._ws), _ptr(flat), st)
            _lib.call("emer_buffer_to_pixels", _ptr(flat), num_rays, Hb, Wb, self.buffer_downscale, _ptr(cand), self.HEIGHT, self.WIDTH,
                      _ptr(self.seed_word), _SALT_CELL, _ptr(img), _ptr(y), _ptr(x), st)
        if advance:
            self._next_seed()
        return img, y, x

    def _support_ok(self, num_rays: int, img_candidate_indices=None) -> bool:
        """True when the cached count of positive cells of the WHOLE error buffer already proves that ``num_rays`` cells can be
        drawn without replacement (candidate subsets fall back to the per-call check)."""
        if img_candidate_indices is not None:
            return False
        ver = self.pixel_error_maps._version
        cache = getattr(self, "_support_cache", None)
        if cache is None or cache[0] != ver or cache[2] is not self.pixel_error_maps:
            cache = self._support_cache = (ver, int((self.pixel_error_maps > 0).sum()), self.pixel_error_maps)
        return num_rays <= cache[1]

    # ---------------------------------------------------------------------------------------------------- rays
    def _gather(self, img_idx: Tensor, y: Tensor, x: Tensor) -> Dict[str, Tensor]:
        n, dev = img_idx.numel(), self.device
        out = {"origins": torch.empty((n, 3), device=dev), "viewdirs": torch.empty((n, 3), device=dev),
               "direction_norms": torch.empty((n, 1), device=dev), "pixel_coords": torch.empty((n, 2), device=dev),
               "pixels": torch.empty((n, 3), device=dev)}
        sky = torch.empty(n, device=dev) if self.sky_masks is not None else None
        ts = torch.empty(n, device=dev) if self.normalized_timestamps is not None else None
        cam = torch.empty(n, dtype=torch.int64, device=dev) if self.cam_ids is not None else None
        with torch.cuda.device(dev):
            _lib.call("emer_gen_rays", _ptr(img_idx), _ptr(y), _ptr(x), _ptr(self.cam_to_worlds), _ptr(self.intrinsics), _ptr(self.images),
                      _ptr(self.sky_masks), _ptr(self.normalized_timestamps), _ptr(self.cam_ids), n, self.HEIGHT, self.WIDTH,
                      _ptr(out["origins"]), _ptr(out["viewdirs"]), _ptr(out["direction_norms"]), _ptr(out["pixel_coords"]),
                      _ptr(out["pixels"]), _ptr(sky), _ptr(ts), _ptr(cam), _stream(img_idx))
        if ts is not None:
            out["normed_timestamps"] = ts
        out["img_idx"] = img_idx
        if cam is not None:
            out["cam_idx"] = cam
        if sky is not None:
            out["sky_masks"] = sky
        if self.dynamic_masks is not None or self.features is not None:
            dyn = torch.empty(n, device=dev) if self.dynamic_masks is not None else None
            feat = None
            Hf = Wf = E = 0
            sy = sx = 0.0
            if self.features is not None:
                _, Hf, Wf, E = self.features.shape
                sy, sx = self.featmap_downscale_factor
                feat = torch.empty((n, E), device=dev)
            with torch.cuda.device(dev):
                _lib.call("emer_gather_pixel_extras", _ptr(img_idx), _ptr(y), _ptr(x), n, self.HEIGHT, self.WIDTH, _ptr(self.dynamic_masks),
                          _ptr(self.features), Hf, Wf, E, sy, sx, _ptr(dyn), _ptr(feat), _stream(img_idx))
            if dyn is not None:
                out["dynamic_masks"] = dyn
            if feat is not None:
                out["features"] = feat
        return out

    def get_train_rays(self, num_rays: int, candidate_indices=None) -> Dict[str, Tensor]:
        """:670-731: ``buffer_ratio`` of the batch from the error buffer (once it exists), the rest uniform."""
        if self.buffer_ratio > 0 and self.pixel_error_buffered:
            n_roi = int(num_rays * self.buffer_ratio)
            ri, ry, rx = self.sample_uniform_rays(num_rays - n_roi, candidate_indices, advance=False)
            # support of the error buffer: one device->host read when the buffer is built / updated (cached), none per step
            bi, by, bx = self.sample_important_rays(n_roi, candidate_indices, advance=False,
                                                    check_support=not self._support_ok(n_roi, candidate_indices))
            img_idx, y, x = torch.cat([ri, bi]), torch.cat([ry, by]), torch.cat([rx, bx])
        else:
            img_idx, y, x = self.sample_uniform_rays(num_rays, candidate_indices, advance=False)
        self._next_seed()
        return self._gather(img_idx, y, x)

    def _lowres_tables(self, s: float):
        if self._resample_tables is None or self._resample_tables[0] != s:
            h, w = int(math.floor(self.HEIGHT * s)), int(math.floor(self.WIDTH * s))
            if not (0 < s < 1.0 and h >= 1 and w >= 1):
                raise ValueError(f"downscale_factor {s}: need 0 < factor <= 1 and at least one output pixel per axis")
            ty, tx = antialias_bicubic_tables(self.HEIGHT, h, s), antialias_bicubic_tables(self.WIDTH, w, s)
            dev_t = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (*ty, *tx))
            self._resample_tables = (s, h, w, ty[2].shape[1], tx[2].shape[1], dev_t)
        return self._resample_tables[1:]

    def _render_rays_lowres(self, img_idx: int, s: float) -> Dict[str, Tensor]:
        """:733-846 at a factor != 1 in one launch (csrc/rays.hip render_rays_lowres_kernel): [h, w] = floor([H, W] * s)."""
        h, w, ky, kx, (ymin, ysize, wy, xmin, xsize, wx) = self._lowres_tables(s)
        dev = self.device
        if not 0 <= int(img_idx) < self.num_imgs:
            raise IndexError(f"get_render_rays: image {img_idx} of {self.num_imgs}")
        out = {"origins": torch.empty((h, w, 3), device=dev), "viewdirs": torch.empty((h, w, 3), device=dev),
               "direction_norm": torch.empty((h, w, 1), device=dev), "pixel_coords": torch.empty((h, w, 2), device=dev)}
        ts = torch.empty((h, w), device=dev) if self.normalized_timestamps is not None else None
        img = torch.empty((h, w), dtype=torch.int64, device=dev)
        cam = torch.empty((h, w), dtype=torch.int64, device=dev) if self.cam_ids is not None else None
        pixels = torch.empty((h, w, 3), device=dev)
        sky = torch.empty((h, w), device=dev) if self.sky_masks is not None else None
        dyn = torch.empty((h, w), device=dev) if self.dynamic_masks is not None else None
        feat, Hf, Wf, E, fsy, fsx = None, 0, 0, 0, 0.0, 0.0
        if self.features is not None:
            _, Hf, Wf, E = self.features.shape
            fsy, fsx = self.featmap_downscale_factor[0] / s, self.featmap_downscale_factor[1] / s   # :803-806
            feat = torch.empty((h, w, E), device=dev)
        with torch.cuda.device(dev):
            _lib.call("emer_render_rays_lowres", int(img_idx), _ptr(self.cam_to_worlds), _ptr(self.intrinsics), _ptr(self.images),
                      _ptr(self.sky_masks), _ptr(self.dynamic_masks), _ptr(self.features), _ptr(self.normalized_timestamps), _ptr(self.cam_ids),
                      self.HEIGHT, self.WIDTH, h, w, s, 1.0 / s, _ptr(ymin), _ptr(ysize), _ptr(wy), ky, _ptr(xmin), _ptr(xsize), _ptr(wx), kx,
                      Hf, Wf, E, fsy, fsx, _ptr(out["origins"]), _ptr(out["viewdirs"]), _ptr(out["direction_norm"]), _ptr(out["pixel_coords"]),
                      _ptr(pixels), _ptr(sky), _ptr(dyn), _ptr(feat), _ptr(ts), _ptr(img), _ptr(cam), _stream(pixels))
        if ts is not None:
            out["normed_timestamps"] = ts
        out["img_idx"] = img
        if cam is not None:
            out["cam_idx"] = cam
        out["pixels"] = pixels
        for k, v in (("sky_masks", sky), ("dynamic_masks", dyn), ("features", feat)):
            if v is not None:
                out[k] = v
        return out

    def get_render_rays(self, img_idx: int) -> Dict[str, Tensor]:
        """:733-846: every pixel of one image, image-shaped tensors (H, W, ...).  At ``downscale_factor`` s != 1 the image is
        [floor(H s), floor(W s)]: colours resampled as torch's antialiased bicubic ``interpolate`` does, masks by its nearest
        mode, rays through the pixel centres of the camera with intrinsics * s, features looked up at the rescaled
        coordinates -- one launch; at 1.0, the full-resolution gather."""
        if self._downscale_factor != 1.0:
            return self._render_rays_lowres(img_idx, float(self._downscale_factor))
        H, W, dev = self.HEIGHT, self.WIDTH, self.device
        if self._all is None:
            yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
            self._all = (yy.reshape(-1).contiguous(), xx.reshape(-1).contiguous())
        y, x = self._all
        out = self._gather(torch.full((H * W,), int(img_idx), dtype=torch.int64, device=dev), y, x)
        out["direction_norm"] = out.pop("direction_norms")   # the reference's render dict spells this key in the singular (:836)
        return {k: v.reshape(H, W, -1).squeeze(-1) if k in ("normed_timestamps", "img_idx", "cam_idx", "sky_masks", "dynamic_masks") else v.reshape(H, W, -1)
                for k, v in out.items()}

    def __len__(self) -> int:
        return self.num_imgs

    # -------------------------------------------------------------------------------------------- scene box (:391-437)
    def get_aabb(self, num_cams: Optional[int] = None) -> Tensor:
        """:391-437 -> the coarse scene box [x0, y0, z0, x1, y1, z1] (fp32, on the device) from the FRONT camera's trajectory: its
        position range, extended by 40 m along x and y, by 20 m upwards (capped at 20) and 5 m downwards (at least down to -5).
        The front camera is image 0, 1, 2 or 2 of every group of 1, 3, 5 or 6 cameras (the orders of the reference's loaders).
        ``num_cams``: default the number of distinct ``cam_ids`` (1 without them).  Plain torch: a handful of numbers once per
        run; the dataset picks this box or the lidar one (``LidarSource.get_aabb``)."""
        if num_cams is None:
            num_cams = 1 if self.cam_ids is None else int(self.cam_ids.unique().numel())
        front = {1: 0, 3: 1, 5: 2, 6: 2}.get(int(num_cams))
        if front is None:
            raise ValueError(f"get_aabb: the front camera is known for 1, 3, 5 or 6 cameras, not {num_cams}")
        pos = self.cam_to_worlds[front::int(num_cams), :3, 3]
        lo, hi = pos.min(dim=0)[0], pos.max(dim=0)[0]
        hi = torch.stack([hi[0] + 40, hi[1] + 40, torch.clamp(hi[2] + 20, max=20.0)])
        lo = torch.stack([lo[0] - 40, lo[1] - 40, torch.clamp(lo[2] - 5, min=-5.0)])
        return torch.cat([lo, hi])

    def __getitem__(self, idx: int) -> Dict[str, Tensor]:
        return self.get_render_rays(idx)

    # -------------------------------------------------------------------------------------------- synthetic data
    @classmethod
    def synthetic(cls, device, num_imgs: int = 50, height: int = 160, width: int = 240, num_cams: int = 1, seed: int = 0,
                  buffer_ratio: float = 0.0, dynamic_ratio: float = 0.0, feature_dim: int = 0,
                  feature_hw: Optional[Tuple[int, int]] = None) -> "PixelSource":
        """A seeded stand-in for a driving log (no dataset on the box): a camera moving along +x through the scene box of
        configs/default_config.yaml, random images, 15 % sky.  ``dynamic_ratio`` > 0: random dynamic masks covering that
        share of the pixels; ``feature_dim`` > 0: random [feature_hw] x feature_dim feature maps (default 1/8 of the image
        size).  Both are drawn after everything else, so the data without them stays the same bit for bit."""
        g = torch.Generator().manual_seed(seed)
        n_t = num_imgs // num_cams
        c2w = torch.eye(4).repeat(num_imgs, 1, 1)
        for i in range(num_imgs):
            t, cam = i // num_cams, i % num_cams
            yaw = (cam - (num_cams - 1) / 2) * 0.7
            # camera looks along world +x (OpenCV camera: z forward, x right, y down)
            fwd = torch.tensor([torch.cos(torch.tensor(yaw)), torch.sin(torch.tensor(yaw)), 0.0])
            right = torch.tensor([fwd[1], -fwd[0], 0.0])
            down = torch.tensor([0.0, 0.0, -1.0])
            c2w[i, :3, 0], c2w[i, :3, 1], c2w[i, :3, 2] = right, down, fwd
            c2w[i, :3, 3] = torch.tensor([60.0 * t / max(n_t - 1, 1), 0.0, 2.0])
        K = torch.tensor([[0.8 * width, 0.0, width / 2], [0.0, 0.8 * width, height / 2], [0.0, 0.0, 1.0]]).repeat(num_imgs, 1, 1)
        images = torch.rand(num_imgs, height, width, 3, generator=g)
        sky = (torch.rand(num_imgs, height, width, generator=g) < 0.15).float()
        ts = (torch.arange(num_imgs) // num_cams).float() / max(n_t - 1, 1)
        cams = torch.arange(num_imgs) % num_cams
        dyn = (torch.rand(num_imgs, height, width, generator=g) < dynamic_ratio).float().to(device) if dynamic_ratio > 0 else None
        feats = None
        if feature_dim > 0:
            hf, wf = feature_hw if feature_hw is not None else (max(height // 8, 1), max(width // 8, 1))
            feats = torch.rand(num_imgs, hf, wf, feature_dim, generator=g).to(device)
        return cls(images.to(device), c2w.to(device), K.to(device), sky.to(device), ts.to(device), cams.to(device),
                   buffer_ratio=buffer_ratio, seed=seed, dynamic_masks=dyn, features=feats)
