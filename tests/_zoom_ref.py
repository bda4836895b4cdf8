"""numpy restatement of the five-view resize (the reference's ``resize_five_views``, utils/visualization_tools.py:36-49; here
``video_utils.compose_video_frames(..., five_view_resize="zoom")``, ``ops.zoom_rows`` / ``ops.five_view_frame``, csrc/frames.hip),
written from the rules and not from the kernel.

The rules.  Of a group of exactly five views, views 0 and 4 become a black [H, W, 3] image whose bottom ``h = int(W * 0.46)`` rows
hold ``scipy.ndimage.zoom(img, [h / H, 1, 1])`` (order 3, ``mode="constant"``, prefilter on, ``grid_mode=False``), clipped to
[0, 1].  Along x and the channel axis the zoom factor is 1 and prefilter plus interpolation at integer positions is the identity
in exact arithmetic, so only the y axis is restated:

  * prefilter of a column of n values with the cubic B-spline pole ``z = sqrt(3) - 2`` and mirror ends (``c[-i] = c[i]``,
    ``c[n-1+i] = c[n-1-i]``): the gain ``(1 - z)(1 - 1/z)`` on every value; ``c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1}^{n-2}
    z^i (c[i] + z^(n-1) c[n-1-i])) / (1 - z^(2(n-1)))``; ``c[i] += z c[i-1]`` upwards; ``c[n-1] = (z c[n-2] + c[n-1]) z /
    (z^2 - 1)``; ``c[i] = z (c[i+1] - c[i])`` downwards;
  * output row y samples at ``cc = fl(fl((H - 1) / (h - 1)) * y)`` -- two fp64 roundings, kept as they are because an ulp of a
    coordinate of a few hundred is worth 1e-13 of a value; with ``f = floor(cc)``, ``t = cc - f``, ``u = 1 - t`` the weights on
    the rows f - 1 .. f + 2 are ``u^3 / 6``, ``(t t (t - 2) 3 + 4) / 6``, ``(u u (u - 2) 3 + 4) / 6`` and one minus their sum,
    and a row index outside the image is mirrored into it.

Types: a colour, mask or sky tile is fp32 and scipy returns the input's type: the fp64 value is ROUNDED TO fp32, clipped, and
cut to 8 bits by the frame's rule (``_frame_ref.to8``).  A depth tile is the fp64 colour of matplotlib's float turbo table (black
for a NaN position) before the zoom; the value stays fp64, is clipped and ``uint8(255 * x)`` is formed in fp64.

The bound.  Every entry comes as ``(v, e)``: the fp64 value of this restatement and ``e = K_ROUND * 2^-53 * sum|w| * 3 *
max|column|``.  ``3 * max|column|`` bounds a coefficient (the prefilter's gain in the maximum norm, reached by a column that
alternates), ``sum|w| = 1`` for the B-spline weights, so the factor behind ``K_ROUND * 2^-53`` bounds every intermediate, and
K_ROUND counts roundings, each taken at that magnitude (a generous unit: most intermediates are smaller):

  scipy, per axis (three axes, two of them the identity up to this noise):
      gain 1; initial value: 3 roundings per term under weights z^i, a geometric sum below 5, and the division 1; the upward
      pass 2 per step, an error made k steps earlier arrives times z^k: below 3; the downward start 4, the downward pass 2 per
      step: below 3; what the upward pass left goes through the downward pass times at most |z| / (1 - |z|) < 1  ... <= 17
      interpolation: the coordinate is exact in both; t, u 2; each weight at most 5, the last 3; 4 products, 3 sums  ... <= 25
    three axes                                                                                                          <= 126
  this restatement or the kernel, y axis only: the same chain once (42), the kernel's block scheme instead of the whole-line
      passes -- the running sum of the downward start, 3 roundings per term under weights z^k: below 5, and the truncation of
      both warm-ups, below 1 (csrc/frames.hip) -- and in a depth tile nothing more (the table entry is exact)            <= 48
                                                                                                          K_ROUND = 126 + 48 -> 176

so a scipy value and a kernel value may each lie ``e`` from ``v`` (each is compared with ``v``, not with the other).  With
values in [-0.2, 1.2] ``e <= 176 * 3.6 * 2^-53 < 2^-43``.  One limit: the noise of scipy's x-axis round trip is proportional to
the values of a ROW, so in an all-zero column beside nonzero ones scipy leaves 1e-16 where ``e`` is 0 (the kernel, which never
mixes columns, gives 0); the scipy comparisons therefore use columns whose magnitude is that of their neighbours.
"""
from __future__ import annotations

import numpy as np

from tests import _frame_ref as R

K_ROUND = 176
POLE = np.sqrt(3.0) - 2.0
FRACTION = 0.46


def out_rows(W):
    """h = int(W * 0.46)."""
    return int(W * FRACTION)


def prefilter_columns(a, mirror=True):
    """The cubic B-spline coefficients along axis 0 of an fp64 [n, ...] array.  ``mirror=False`` is a mutant (ends that see
    zeros outside the image instead of the mirror image)."""
    z = POLE
    c = np.array(a, dtype=np.float64) * ((1 - z) * (1 - 1 / z))
    n = c.shape[0]
    assert n >= 2
    if mirror:
        zn = z ** (n - 1)
        c0 = c[0] + zn * c[n - 1]
        zi = z
        for i in range(1, n - 1):
            c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
            zi *= z
        c[0] = c0 / (1 - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    if mirror:
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
    else:
        c[n - 1] = -z * c[n - 1]
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def mirror_index(i, n):
    m = np.mod(i, 2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def zoom_columns(a, h, mirror=True, rule="scipy"):
    """(v, e) of the y-axis zoom of an [H, ...] array to h rows, fp64.  ``rule="grid"`` is a mutant (the H / h coordinate rule)."""
    a = np.asarray(a, dtype=np.float64)
    H = a.shape[0]
    if not 2 <= h <= H:
        raise ValueError(f"h = {h} rows from H = {H}")
    with np.errstate(all="ignore"):
        c = prefilter_columns(a, mirror)
        zoom = np.float64(H - 1) / np.float64(h - 1) if rule == "scipy" else np.float64(H) / np.float64(h)
        cc = zoom * np.arange(h, dtype=np.float64)
        f = np.floor(cc)
        t = cc - f
        u = 1.0 - t
        w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
        w0 = u * u * u / 6.0
        w3 = 1.0 - w0 - w1 - w2
        f = f.astype(np.int64)
        shape = (h,) + (1,) * (a.ndim - 1)
        v = np.zeros((h,) + a.shape[1:], dtype=np.float64)
        sw = np.zeros(h)
        for k, w in enumerate((w0, w1, w2, w3)):
            v = v + c[mirror_index(f - 1 + k, H)] * w.reshape(shape)
            sw = sw + np.abs(w)
        e = K_ROUND * 2.0 ** -53 * sw.reshape(shape) * 3.0 * np.max(np.abs(a), axis=0, keepdims=True)
    return v, np.broadcast_to(e, v.shape)


def depth_colour_sets(depth, opacity, table64, lo=R.LO, hi=R.HI):
    """The fp64 [H, W, 3] turbo colours of a depth image, for each of the three logarithm choices of ``_frame_ref``."""
    lut = np.concatenate([np.asarray(table64, dtype=np.float64).reshape(256, 3), np.zeros((1, 3))])
    return tuple(lut[r] for r in R.depth_row_sets(depth, opacity, lo, hi))


def tile_source(kind, src, opacity, table64, lo=R.LO, hi=R.HI):
    """What the zoom of a tile reads, as (fp64 [H, W, 3] or [H, W] array, is_fp64_tile): the mask kinds stay one channel."""
    if kind == "colour3":
        return np.asarray(src, dtype=np.float32).astype(np.float64), False
    if kind == "grey1":
        return np.asarray(src, dtype=np.float32).astype(np.float64), False
    if kind == "one_minus_grey1":
        return (np.float32(1) - np.asarray(src, dtype=np.float32)).astype(np.float64), False
    if kind == "depth":
        return depth_colour_sets(src, opacity, table64, lo, hi)[0], True
    raise ValueError(kind)


def zoom_values(kind, src, opacity, h, table64, lo=R.LO, hi=R.HI, **mutant):
    """(v, e) as [h, W, 3] fp64: what ``ops.zoom_rows`` returns and its bound."""
    a, _ = tile_source(kind, src, opacity, table64, lo, hi)
    v, e = zoom_columns(a, h, **mutant)
    if v.ndim == 2:
        v, e = np.repeat(v[..., None], 3, axis=-1), np.repeat(e[..., None], 3, axis=-1)
    return v, np.array(e)


def bytes_of(x, is_fp64_tile, fp64_scale, round32=True):
    """8 bits of zoomed values.  ``round32=False`` is a mutant (no rounding to fp32 before the clip)."""
    with np.errstate(all="ignore"):
        if is_fp64_tile or not round32:
            y = 255 * np.clip(x, 0, 1) if (is_fp64_tile or fp64_scale) else (np.float32(255) * np.clip(x, 0, 1).astype(np.float32))
            return np.where(np.isnan(y), 0, y).astype(np.uint8)
        return R.to8(np.asarray(x, dtype=np.float64).astype(np.float32), fp64_scale)


def resized_tile8(kind, src, opacity, fp64_scale, table64, lo=R.LO, hi=R.HI, round32=True, **mutant):
    """The three [H, W, 3] uint8 versions of a resized view: black above, the bytes of v, v - e and v + e below."""
    H, W = np.asarray(src).shape[:2]
    h = out_rows(W)
    v, e = zoom_values(kind, src, opacity, h, table64, lo, hi, **mutant)
    out = []
    for x in (v, v - e, v + e):
        t = np.zeros((H, W, 3), np.uint8)
        t[H - h:] = bytes_of(x, kind == "depth", fp64_scale, round32)
        out.append(t)
    return tuple(out)


def compose(tiles, H, W, rows, cams, fp64, table8, table64, lo=R.LO, hi=R.HI, **mutant):
    """``_frame_ref.compose`` with the five-view rule: in a frame of five columns the tiles of columns 0 and 4 are resized.  The
    three frames: (t, v), (t - d, v - e), (t + d, v + e) -- a pixel is either a depth pixel of a middle view or a resized one."""
    def resized(t):
        return cams == 5 and t[2] in (0, 4)
    out = R.compose([t for t in tiles if not resized(t)], H, W, rows, cams, fp64, table8, lo, hi)
    for kind, r, c, src, opacity in filter(resized, tiles):
        for o, t in zip(out, resized_tile8(kind, src, opacity, fp64, table64, lo, hi, **mutant)):
            o[r * H:(r + 1) * H, c * W:(c + 1) * W] = t
    return out


def video_frames(results, num_timestamps, keys, num_cams, separate, table8, table64, **mutant):
    """``_frame_ref.video_frames`` with the five-view rule."""
    plan = R.frame_plan(results, keys, separate)
    out = []

    def frame(rows, i, fp64):
        tiles = []
        for r, (_, kind, images, opacities) in enumerate(rows):
            for c, x in enumerate(images[i * num_cams:(i + 1) * num_cams]):
                tiles.append((kind, r, c, np.asarray(x), None if opacities is None else np.asarray(opacities[i * num_cams + c])))
        H, W = tiles[0][3].shape[:2]
        cams = len(rows[0][2][i * num_cams:(i + 1) * num_cams])
        return compose(tiles, H, W, len(rows), cams, fp64, table8, table64, **mutant)

    if separate:
        for row in plan:
            for i in range(num_timestamps):
                out.append(((row[0], i), frame([row], i, False)))
    else:
        fp64 = any(kind == "depth" for _, kind, _, _ in plan)
        for i in range(num_timestamps):
            out.append(((i,), frame(plan, i, fp64)))
    return out
