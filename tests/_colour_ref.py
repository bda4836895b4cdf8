"""float64 numpy restatements of the three evaluation-colour formulas (csrc/colours.hip; the reference's
radiance_fields/video_utils.py:233-418 and utils/visualization_tools.py:204-275) with the per-entry bounds the fp32
implementations -- the kernels AND the reference's own torch / numpy chains -- are held to.  Derived in the manner of
tests/_bounds.py, not fitted: u = 2^-24 is the unit roundoff of fp32, every fp32 operation returns its exact result times
(1 + delta), |delta| <= u, and terms of second order in u are covered by the slack named in each derivation.
"""
import numpy as np

U = 2.0 ** -24
FLOW_BOUND = 1e-5
N_COLS = 55            # wheel steps; the wheel has N_COLS + 1 rows (the first repeated)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def clamp01(x):
    """torch.clamp(x, 0, 1) / np.clip: +-inf clamp, NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))


def feature_colours(feat, mat, lo, hi, scale=None):
    """(colours, bound): clamp((feat @ mat - lo) / (hi - lo), 0, 1) [* scale] in float64 of the fp32 inputs, and the bound

        |got - ref| <= u ((E + 2) A / |d| + 5 |x|) [+ u |x|],   A = sum_e |f_e M[e, c]|,  d = hi_c - lo_c,  x before the clamp.

    Terms: p = sum_e f_e M[e, c] from E products and E - 1 additions in ANY order (or fma chains: fewer roundings) is off by at
    most (E u) A to first order; the subtraction p - lo adds u |p - lo|, the rounding of d adds u |x|, the division u |x|: in
    units of x that is u (E A / |d| + 3 |x|).  |p - lo| / |d| = |x| exactly, so two of the five |x| and the two extra A / |d|
    are slack (second-order terms, and one unit as the issue states).  clamp is 1-Lipschitz and the scale s in [0, 1] shrinks
    the error; its product rounds once more: + u |x|.  Where d == 0 the quotient is +-inf (clamps exactly) or 0 / 0 = NaN:
    the bound is inf there and the caller compares those entries exactly."""
    f, m, lo, hi = _f64(feat), _f64(mat), _f64(lo).reshape(3), _f64(hi).reshape(3)
    E = f.shape[-1]
    f = f.reshape(-1, E)
    d = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (f @ m - lo) / d
        A = np.abs(f) @ np.abs(m)
        bound = U * ((E + 2) * A / np.abs(d) + 5 * np.abs(x))
        y = clamp01(x)
        if scale is not None:
            s = _f64(scale).reshape(-1, 1)
            y = y * s
            bound = bound + U * np.abs(x)
    return y, bound


def blend_over(a, o, b, bound_a=0.0, bound_b=0.0):
    """(clip(a o + b (1 - o), 0, 1), bound) in float64: three roundings on the first product's path (product, sum) and four on the
    second's (1 - o, product, sum) give at most 4 u (|a o| + |b (1 - o)|) with the second-order terms inside the slack of the
    first path; the inputs' own bounds pass through weighted by |o| and |1 - o|; the clip is 1-Lipschitz."""
    a, b = _f64(a).reshape(-1, 3), _f64(b).reshape(-1, 3)
    o = _f64(o).reshape(-1, 1)
    t0, t1 = a * o, b * (1.0 - o)
    bound = 4 * U * (np.abs(t0) + np.abs(t1)) + np.abs(o) * bound_a + np.abs(1.0 - o) * bound_b
    return clamp01(t0 + t1), bound


def flow_colours(flow, wheel, max_radius=1.0, background="bright"):
    """scene_flow_to_rgb(flow, flow_max_radius=max_radius, background) in float64; [N, 3] in [0, 1].  FLOW_BOUND = 1e-5 on the
    colours holds for any fp32 evaluation of the same steps:

      * the angle index a = angle (N_COLS - 1) / 2 pi <= 54 carries atan2's error (a few u relative), the + 2 pi, the rounding
        of the constant and the product: at most about 6 u * 54 = 1.9e-5 index units;
      * the hue is piecewise linear and CONTINUOUS in a (at a node both neighbours give the node's colour, so a trunc / ceil
        landing on the other side of a node in fp32 costs nothing); its steepest transition moves 255 / 4 per index unit, i.e.
        0.25 per unit on the [0, 1] scale: 1.9e-5 * 0.25 = 4.8e-6;
      * the radius factor is <= 1 on both sides of radius = 1 and the map is continuous there (both branches give the hue at
        radius 1), so the hue's error is not amplified; hypot, the division by the radius and the S / V move are a few
        roundings of values <= 255, i.e. <= about 6 u * 255 / 255 = 3.6e-7 each on the [0, 1] scale, say 2e-6 together;
      * the interpolation's two products and sum: 3 u * 255 / 255 = 1.8e-7.

    Together about 7e-6 < 1e-5."""
    f = _f64(flow).reshape(-1, 3)
    w = _f64(wheel)
    assert w.shape == (N_COLS + 1, 3) and background in ("bright", "dark")
    x, y = f[:, 0], f[:, 1]
    radius, angle = np.hypot(x, y), np.arctan2(y, x)
    if max_radius > 0:
        radius = radius / max_radius
    angle = np.where(angle < 0, angle + 2 * np.pi, angle) * ((N_COLS - 1) / (2 * np.pi))
    frac = np.fmod(angle, 1.0)[:, None]
    i0, i1 = np.trunc(angle).astype(np.int64), np.ceil(angle).astype(np.int64)
    hue = w[i0] * (1 - frac) + w[i1] * frac
    r = radius[:, None]
    big = r > 1
    with np.errstate(divide="ignore"):
        factor = np.where(big, 1.0 / r, r)
    s_axis, v_axis = 255.0 - factor * (255.0 - hue), hue * factor
    if background == "dark":
        col = np.where(big, s_axis, v_axis)
    else:
        col = np.where(big, v_axis, s_axis)
    return col / 255.0


def lower_median(x, axis=0):
    """torch.median: the lower of the two middle values for an even count."""
    s = np.sort(x, axis=axis)
    return np.take(s, (x.shape[axis] - 1) // 2, axis=axis)


def robust_range(colors, m):
    """utils/misc.py:38-46 on [N, 3] colours: per channel, min and max over the rows whose absolute deviation from the median is
    below m median absolute deviations."""
    c = np.asarray(colors)
    d = np.abs(c - lower_median(c))
    s = d / lower_median(d)
    lo = np.array([c[s[:, k] < m, k].min() for k in range(3)])
    hi = np.array([c[s[:, k] < m, k].max() for k in range(3)])
    return lo, hi


def assert_within(got, ref, bound, tag):
    """|got - ref| <= bound per entry; NaN exactly where ref has NaN; entries with an infinite bound (d == 0) compared exactly."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(ref.shape), np.asarray(ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), f"{tag}: NaN pattern differs"
    exact = ~np.isfinite(bound) & ~nan
    assert (got[exact] == ref[exact]).all(), f"{tag}: entries without a finite bound differ"
    ok = ~nan & ~exact
    err = np.abs(got[ok] - ref[ok])
    worst = (err / np.maximum(bound[ok], 1e-300)).max() if err.size else 0.0
    print(f"{tag}: max err {err.max() if err.size else 0.0:.3e}, worst err / bound {worst:.3f}")
    assert (err <= bound[ok]).all(), f"{tag}: {int((err > bound[ok]).sum())} entries beyond the bound (worst {worst:.2f} x)"
