"""Double-precision restatement of the low-resolution render path and its error bounds (test helper, not a test module).

``get_render_rays`` at a downscale factor s resamples the colours as torch's ``interpolate(scale_factor=s, mode="bicubic",
antialias=True)`` and the masks as its ``mode="nearest"``.  Per axis, for output i of ``out = floor(in * s)``:

    support 2 / s, centre c = (i + 0.5) / s, window [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), in)),
    tap weight cubic((j - c + 0.5) * s) (Keys, a = -0.5), normalised over the window actually used;
    nearest source index min(floor(float32(i) * float32(1 / s)), in - 1).

A result is held, entry by entry, to ``|got - ref| <= c * 2^-24 * abs_sum`` with ``abs_sum = sum |w_y| |w_x| |x|`` and ``c``
DERIVED from the accumulation structure of the code under test by counting fp32 roundings (each of relative error
<= u = 2^-24), in the style of tests/_bounds.py -- never fitted to a measured error.  An entry whose abs_sum is 0 must be
exactly 0.  Every ``c`` carries one unit of slack for second-order terms and for a window edge that moves by one tap between
float32 and float64 (such a tap sits at |argument| = 2, a double root of the cubic: its weight is second order in the
rounding).
"""
import numpy as np

U = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------- restatement
def out_size(in_size: int, s: float) -> int:
    return int(np.floor(in_size * s))


def _pieces(x, a):
    """cubic(x), the sum of the absolute values of its Horner terms, and |cubic'(x)| (x >= 0)."""
    inner = x < 1.0
    mid = (x >= 1.0) & (x < 2.0)
    w = np.where(inner, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(mid, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    mag = np.where(inner, ((abs(a + 2) * x + abs(a + 3)) * x * x + 1), np.where(mid, (((x + 5) * x + 8) * x + 4) * abs(a), 0.0))
    der = np.where(inner, np.abs(3 * (a + 2) * x * x - 2 * (a + 3) * x), np.where(mid, np.abs(a * (3 * x * x - 10 * x + 8)), 0.0))
    return w, mag, der


def axis_weights(in_size: int, s: float, a: float = -0.5, mapping: str = "1/s", renormalise: bool = True):
    """(W [out, in] float64 dense weight matrix, taps [out] window sizes, E [out, in] absolute error bound, in units of u, of
    the same weights computed in float32 as torch's CPU kernel computes them -- see c_torch_separable).

    Mutants for the tests: ``a`` (torch's non-antialiased bicubic uses -0.75), ``mapping="in/out"`` (the coordinate scale
    in / out instead of 1 / s; they differ when in * s is not an integer), ``renormalise=False`` (weights divided by the total
    of the whole window, including the taps that fall outside the image)."""
    n_out = out_size(in_size, s)
    inv = 1.0 / s if mapping == "1/s" else in_size / n_out
    arg_scale = s if mapping == "1/s" else 1.0 / inv
    support = 2.0 * inv
    W = np.zeros((n_out, in_size))
    E = np.zeros((n_out, in_size))
    taps = np.zeros(n_out, dtype=np.int64)
    for i in range(n_out):
        c = (i + 0.5) * inv if mapping != "1/s" else (i + 0.5) / s
        lo_full, hi_full = int(c - support + 0.5), int(c + support + 0.5)
        lo, hi = max(lo_full, 0), min(hi_full, in_size)
        j_full = np.arange(min(lo_full, lo), max(hi_full, hi), dtype=np.float64)
        t2 = j_full - c + 0.5
        x = np.abs(t2 * arg_scale)
        w, mag, der = _pieces(x, a)
        inside = (j_full >= lo) & (j_full < hi)
        total = w[inside].sum() if renormalise else w.sum()
        W[i, lo:hi] = w[inside] / total
        taps[i] = hi - lo
        # float32 evaluation (units of u): the argument passes centre = scale * (i + 0.5), j - centre, + 0.5, * invscale (invscale
        # itself rounded): dx <= (|c| + |j - c| + |t2|) / inv + 2 |x|; the polynomial at most 6 operations on terms of total
        # magnitude `mag`, plus |cubic'| dx; the total n - 1 additions of the weights; the division one more
        dx = (abs(c) + np.abs(j_full - c) + np.abs(t2)) / inv + 2 * x
        e = (6 * mag + der * dx)[inside]
        d_total = e.sum() + (hi - lo - 1) * np.abs(w[inside]).sum()
        E[i, lo:hi] = e / abs(total) + np.abs(W[i, lo:hi]) * (d_total / abs(total) + 1)
    return W, taps, E


def nearest_index(in_size: int, s: float) -> np.ndarray:
    """torch's mode="nearest" with a scale factor: float32 product of the output index and float32(1 / s), floored."""
    n_out = out_size(in_size, s)
    scale = np.float32(1.0 / s)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def resample(image: np.ndarray, s: float, **mutant):
    """image [H, W, C] -> dict(ref [h, w, C], abs_sum, ny [h], nx [w], weight_err): float64.  ``weight_err`` is
    sum (E_y |w_x| + |w_y| E_x) |x| in units of u (see c_torch_separable)."""
    H, W = image.shape[:2]
    x = image.astype(np.float64)
    Wy, ny, Ey = axis_weights(H, s, **mutant)
    Wx, nx, Ex = axis_weights(W, s, **mutant)
    ein = lambda A, X, B: np.einsum("ij,jkc,lk->ilc", A, X, B)
    return dict(ref=ein(Wy, x, Wx), abs_sum=ein(np.abs(Wy), np.abs(x), np.abs(Wx)), ny=ny, nx=nx,
                weight_err=ein(Ey, np.abs(x), np.abs(Wx)) + ein(np.abs(Wy), np.abs(x), Ex))


# ---------------------------------------------------------------------------------------------------- derivations of c
def c_resample(ny: np.ndarray, nx: np.ndarray) -> np.ndarray:
    """render_rays_lowres_kernel (csrc/rays.hip), per output entry [h, w, 1]:

    * the weight tables are computed in double precision and rounded to fp32 once: one rounding per axis        -> 2;
    * vertical pass: one serial chain acc = fmaf(w_y, x, acc) from 0 over the ny taps of the row; a term passes through at
      most ny roundings (its own fma and the ones after it), each relative to a partial sum <= abs_sum            -> ny;
    * horizontal pass over the LDS row: the same chain over the nx taps of the column                           -> nx;
    * slack (module docstring)                                                                                    -> 1.

    c = ny + nx + 3."""
    return (ny[:, None] + nx[None, :] + 3).astype(np.float64)[..., None]


def c_torch_separable(r: dict) -> np.ndarray:
    """torch's CPU kernel (separable: the horizontal pass into a temporary, then the vertical pass), float32 throughout, per
    entry of ``resample``'s result:

    * accumulation: each pass forms t = sum w * x term by term (a product and an addition per tap, in any order): a term passes
      through at most n roundings per pass                                                                  -> nx + ny;
    * the WEIGHTS are float32 results of float32 arithmetic, and not every one is accurate relative to itself: the cubic is
      evaluated by Horner's rule, whose error is relative to the magnitude of its terms (2 - 8), while the weight vanishes at
      |x| = 1 and 2; and for s = 1/3 the argument itself is rounded.  ``axis_weights`` carries a first-order running error
      bound E (absolute, units of u) of every normalised weight through exactly the steps torch takes; its contribution to an
      entry is sum (E_y |w_x| + |w_y| E_x) |x| = weight_err, expressed in units of abs_sum                    -> weight_err / abs_sum;
    * slack                                                                                                   -> 1.

    For power-of-two factors the arguments and Horner terms are exact in float32 and the bound is merely loose."""
    a = r["abs_sum"]
    rel = np.divide(r["weight_err"], a, out=np.zeros_like(a), where=a > 0)
    return (r["ny"][:, None] + r["nx"][None, :] + 1).astype(np.float64)[..., None] + rel


# ----------------------------------------------------------------------------------------------- error-buffer refresh
def pixel_error_ref(pred: np.ndarray, gt: np.ndarray, opacity=None):
    """update_pixel_error_maps in float64 and the per-cell bound (absolute) for an fp32 evaluation.

    e = mean_c |gt - pred|: three subtractions (1 rounding each, relative to their own term), two additions (2), the division
    by 3 (1) -> 4 roundings; x 5 where the opacity exceeds 0.1 -> 1 more: e_hat = e (1 + theta_k), k = 5.  With m, M the
    extrema (taken over the same fp32 values, so each carries its own cell's k roundings), v = (e - m) / (M - m) takes 3 more:
    the subtraction e - m, the subtraction M - m, the division.  First order:

        |v_hat - v| <= u [ k (e + m) / (M - m)  +  v ( k (M + m) / (M - m) + 3 ) ]  (+ u slack)."""
    e = np.abs(gt.astype(np.float64) - pred.astype(np.float64)).mean(axis=-1)
    if opacity is not None:
        e = np.where(opacity.reshape(e.shape) > np.float32(0.1), e * 5, e)
    m, M = e.min(), e.max()
    v = (e - m) / (M - m)
    k = 5.0
    bound = U * (k * (e + m) / (M - m) + v * (k * (M + m) / (M - m) + 3) + 1)
    return v, bound
