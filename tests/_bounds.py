"""Per-entry error bounds for the grid kernels (test helper, not a test module).

A kernel that forms the terms of a sum in fp32 and adds them in some order is held, entry by entry, to

    |got - ref| <= c * 2^-24 * abs_sum

where ``ref`` and ``abs_sum`` (the sum of the terms' absolute values) come from the double-precision oracle entry points
(oracle.hashgrid_fwd_bound / hashgrid_bwd_params_bound / hashgrid_bwd_input_bound), and ``c`` counts the fp32 roundings a
term can pass through on the path under test (each rounding has relative error <= u = 2^-24).  ``c`` is DERIVED from the
kernel's accumulation structure in the ``c_*`` functions below, never fitted to a measured error.  An entry whose abs_sum is
0 (untouched, touched only by zero weights or by zero-dOut rows) must come out exactly 0.

Every ``c`` carries one unit of slack for what the first-order count leaves out: second-order terms (gamma_k = k u / (1 - k u)
exceeds k u by less than 1e-5 relative for k < 200), the oracle's own double rounding and the double LDS accumulators of the
owner-computes backward (hits * 2^-53 relative, below 2^-24 for fewer than 2^29 hits).
"""
import ctypes

import numpy as np
import torch

U = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------- derivations of c
# Shared by every path: a term's weight is prod_d t_d with t_d = w_d (exact: pos - floor(pos)) or 1 - w_d (one rounding);
# D factors -> at most D subtractions + D - 1 products = 2D - 1 roundings.


def c_forward(D: int) -> float:
    """hashgrid_fwd_kernel (generic and paired-gather loops): wt (2D - 1), wt * v (1), acc += over 2^D corners starting
    from 0 (2^D - 1), slack 1  ->  2^D + 2D."""
    return float((1 << D) + 2 * D)


def c_input_grad(D: int, L: int, F: int) -> float:
    """d enc / d x, both paths, against sum |scale prod w| |go| (|e1| + |e0|):
    gather (hashgrid_bwd_input_kernel): s = sum_f go v (F: product + F - 1 adds), s1 - s0 (1), wt = scale * D - 1 factors
    (2D - 2), wt * diff (1), acc over 2^(D-1) corner pairs (2^(D-1) - 1), gx over L levels (L - 1);
    stored Jacobian (fwd_jac + bwd_input_jac): v1 - v0 (1), wt (2D - 2), * (1), sum over 2^(D-1) pairs (2^(D-1) - 1),
    go * J (1), over F (F - 1), over L (L - 1).  Both: F + 2D + 2^(D-1) + L - 2; slack 1."""
    return float(F + 2 * D + (1 << (D - 1)) + L - 1)


def c_atomic(D: int, hits: np.ndarray) -> np.ndarray:
    """emer_hashgrid_bwd_params (tcnn-style fp32 global atomics): a term is wt * go (2D roundings) and is then added to
    the entry by one of `hits` fp32 atomics in arbitrary order (at most hits roundings each seeing the whole partial sum):
    hits + 2D, + 2 for the other side's association and slack  ->  hits + 2D + 3 per entry (the issue's recipe)."""
    return hits.astype(np.float64) + (2 * D + 3)


def sliced_plan(desc, L: int):
    """(n_slices, n_ranges) per level of the owner-computes backward (host arithmetic of the library, no GPU)."""
    from emernerf_amd import _lib
    ns, nr = (ctypes.c_uint32 * L)(), (ctypes.c_uint32 * L)()
    rc = _lib.load().emer_hashgrid_sliced_plan(ctypes.byref(desc), ns, nr)
    assert rc > 0, "grid does not take the owner-computes backward"
    return np.array(ns[:L], np.int64), np.array(nr[:L], np.int64)


def c_sliced(meta, desc, hits: np.ndarray, accumulate: bool = False) -> np.ndarray:
    """hashgrid_bwd_params_sliced_kernel, per ENTRY (hits: the oracle's (sample, corner) terms per entry):

    * term wt * go: 2D roundings (+ 2 for the other side's association of the D factors and slack)   -> 2D + 2;
    * levels whose runs of equal cells are summed in fp32 by the segmented DPP scan before the LDS (dense levels, and the
      paired hashed levels -- power-of-two size -- with F >= 2: add_pair_runs): a 64-lane Hillis-Steele scan puts every
      value through at most log2 64 additions                                                          -> + 6;
    * the double LDS accumulators: below the slack (module docstring);
    * write-out: the double sum is rounded to fp32 once per work item (relative to that item's partial: 1 in total); a
      level cut in R sample ranges (dense levels, the tail-split items of the xyzt tables) merges its k <= min(R, hits)
      non-zero partials with fp32 atomics into a zeroed level: k - 1 roundings                          -> + min(R, hits);
    * sliced_add (accumulate): the write-out adds onto the value already there: one rounding more       -> + 1.

    -> c = 2D + 2 + 6 [run-reduced] + min(R, hits) + [accumulate].  The R = 128 sample ranges of a coarse dense level make
    its entries the only ones above 64 (c = 142 for D = 3): the merge of 128 partials is the whole bound there."""
    D, L, F = meta.n_dims, meta.n_levels, meta.n_features
    _, nr = sliced_plan(desc, L)
    c = np.empty(meta.n_entries, np.float64)
    for l in range(L):
        a, b = int(meta.offset[l]), int(meta.offset[l]) + int(meta.size[l])
        size = int(meta.size[l])
        pow2 = size & (size - 1) == 0
        run = (not meta.hashed[l]) or (pow2 and F >= 2)
        c[a:b] = 2 * D + 2 + (6 if run else 0) + np.minimum(hits[a:b].astype(np.float64), float(nr[l])) + (1 if accumulate else 0)
    return c


# fp16 gradient tables: hashgrid_bwd_params_kernel<D, F, __half> (emer_hashgrid_bwd_params with EMER_F16, packed half2 atomics).
# A term wt * go is formed in fp32 (2D roundings at u = 2^-24), converted to half (one rounding at u16 = 2^-11) and added to the
# entry by one of `hits` half atomics in arbitrary order; every addition rounds a partial sum to half.  By the usual induction
# (every term passes its conversion and at most `hits` additions; partial sums of the rounded terms included) the relative
# part is
#
#     |got - ref| <= ((1 + 2D u) (1 + gamma_k) - 1) abs_sum,   gamma_k = k u16 / (1 - k u16),   k = hits + 1 (+ extra)
#
# which needs k u16 < 1 (asserted: fewer than 2047 hits).  ``extra``: further half roundings the value passes on the route
# under test (a cast of the finished gradient).  The absolute part, (hits + 1) 2^-14 per entry, is for results below the normal
# half range (2^-14): whether the packed half atomic of this device keeps or flushes them has not been measured; a kept
# subnormal is off by at most 2^-25 per operation, a flushed one by less than 2^-14, and the term allows one such loss per
# addition and one for the value read back.  The bound is meant for gradients of order 1 - 10 (what loss scale 128 produces),
# where the relative part dominates; the exact probes of tests/test_hashgrid_instances_gpu.py do not depend on it.  Half sums
# overflow at 65504: asserted here from abs_sum (every partial sum is at most (1 + gamma_k) abs_sum).
#
# Measured worst err / bound on an MI355X (tests/test_hashgrid_instances_gpu.py; the atomic order varies from run to run):
#   half atomics, n = 4099, |dOut| in [1, 10], the even-F grids of GRIDS (fp16_atomic_bound)        0.635 (cfg2_static)
#   Encoding(dtype=float16).forward, even F, n = 1000 (fp16_atomic_bound, extra = 1)                 0.427 (D = 4, F = 4)
#   half gradients of an odd feature count, n = 1000 (c_sliced, half_rounded_bound)                  0.996 (the one half rounding:
#       its error reaches 2^-11 of the value at the bottom of a binade, so this ratio sits just below 1 by construction)
#   fp32 atomics, n = 4099, every grid of GRIDS, both dOut layouts (c_atomic)                        0.302 (dynamic_xyzt)
#   gather input gradient with an fp16 table, n = 4099, every grid of GRIDS (c_input_grad)           0.197 (tiny_2d_f1)
#   hashgrid_encode_lm(table_dtype=float16, skip_dx_rows): input gradient (c_input_grad) 0.050, master gradient (c_sliced) 0.211
U16 = 2.0 ** -11
HALF_MIN_NORMAL = 2.0 ** -14
HALF_MAX = 65504.0


def fp16_atomic_bound(D: int, hits: np.ndarray, abs_sum: np.ndarray, extra: int = 0) -> np.ndarray:
    """Per table VALUE (entry, feature) error bound of the half-atomic backward, as an absolute error (see above);
    0 where abs_sum is 0: such an entry must come out exactly 0."""
    hits = np.asarray(hits, np.float64)
    abs_sum = np.asarray(abs_sum, np.float64).reshape(-1)
    F = abs_sum.size // hits.size
    assert F * hits.size == abs_sum.size
    k = np.repeat(hits, F) + 1.0 + extra
    assert float(k.max()) * U16 < 1.0, f"gamma_k needs k u < 1: {int(k.max())} roundings at u = 2^-11"
    gamma = k * U16 / (1.0 - k * U16)
    assert float(((1.0 + gamma) * abs_sum).max()) <= HALF_MAX, "a half partial sum may overflow"
    rel = (1.0 + 2 * D * U) * (1.0 + gamma) - 1.0
    return np.where(abs_sum > 0, rel * abs_sum + (np.repeat(hits, F) + 1.0) * HALF_MIN_NORMAL, 0.0)


def half_rounded_bound(err: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """A value within ``err`` of ``ref`` that is then rounded to half once (round to nearest, subnormals kept: torch's
    cast): u16 of the value before the cast, or half a subnormal step (2^-25); 0 stays 0."""
    err, ref = np.asarray(err, np.float64), np.abs(np.asarray(ref, np.float64))
    return np.where(err > 0, err + np.maximum(U16 * (ref + err), 2.0 ** -25), 0.0)


# ---------------------------------------------------------------------------------------------------------- assertion
def _level_of_entry(meta, e: int) -> int:
    return int(np.searchsorted(meta.offset.astype(np.int64), e, side="right") - 1)


def assert_bound(got, ref, abs_sum, c, what: str, meta=None, kind: str = "params", hits=None, report: dict = None) -> float:
    """|got - ref| <= c 2^-24 abs_sum for every entry (``c`` scalar, or per table entry for kind="params").  kind: "params"
    (flat table gradient), "fwd" ([N, L*F] row-major encoding), "dx" ([N, D]).  Prints and returns the worst err / bound over
    the entries with a non-zero bound; on failure names the worst entry: index, level, hits, abs_sum and err / bound."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    abs_sum = np.asarray(abs_sum, np.float64).reshape(-1)
    assert got.shape == ref.shape == abs_sum.shape, (got.shape, ref.shape, abs_sum.shape)
    F = meta.n_features if meta is not None else 1
    c = np.asarray(c, np.float64)
    if c.ndim and c.size != got.size:   # per table entry -> per (entry, feature)
        c = np.repeat(c, F)
    bound = c * U * abs_sum
    err = np.abs(got - ref)
    bad = ~(err <= bound)                 # (NaN in got fails too)
    pos = bound > 0
    ratio = np.zeros_like(err)
    ratio[pos] = err[pos] / bound[pos]
    worst = float(ratio.max()) if ratio.size else 0.0

    def where(i):
        s = f"index {i}"
        if meta is not None and kind == "params":
            e = i // F
            lv = _level_of_entry(meta, e)
            s += f" (entry {e}, feature {i % F}, level {lv}{', hashed' if meta.hashed[lv] else ', dense'}"
            if hits is not None:
                s += f", hits {int(hits[e])}"
            s += ")"
        elif meta is not None and kind == "fwd":
            row, col = divmod(i, meta.n_output_dims)
            s += f" (row {row}, level {col // F}, feature {col % F})"
        elif meta is not None and kind == "dx":
            s += f" (row {i // meta.n_dims}, dim {i % meta.n_dims})"
        cc = float(c.reshape(-1)[i]) if c.ndim else float(c)
        return s + f": got {got[i]:.9e}, ref {ref[i]:.9e}, abs_sum {abs_sum[i]:.3e}, c {cc:g}, err {err[i]:.3e}"

    if bad.any():
        i = int(np.argmax(np.where(bad, np.where(pos, ratio, np.inf), -1.0)))
        n_zero_bad = int((bad & ~pos).sum())
        raise AssertionError(f"{what}: {int(bad.sum())} entries outside c 2^-24 abs_sum ({n_zero_bad} of them with abs_sum 0 but "
                             f"non-zero); worst {where(i)}, err/bound {ratio[i] if pos[i] else float('inf'):.3g}")
    i = int(np.argmax(ratio)) if ratio.size else 0
    print(f"\n[bound] {what}: worst err/bound {worst:.3f}" + (f" at {where(i)}" if ratio.size and worst > 0 else ""))
    if report is not None:
        report[what] = worst
    return worst


# ------------------------------------------------------------------------------------------------- MLP head kernels
# The heads' GEMMs (csrc/mlp.hip, csrc/mlp_fused.hip) are held to the same form: a layer's own error is at most
# c u abs_sum with abs_sum = sum_k |a| |b| + |bias|, and the error its inputs already carry is propagated to first order
# through |W| (ReLU is 1-Lipschitz, sigmoid 1/4-Lipschitz, exp multiplies by its value).  ``head_*`` below do this
# propagation in fp64 torch, next to the fp64 reference values, and ``assert_head_bound`` checks every entry; an entry whose
# bound is 0 must come out exactly 0.
#
# Assumption: how one MFMA instruction rounds its internal sum on MI355X has not been measured, so every c below counts
# one round-to-nearest rounding PER ADDITION (a sum of n terms in any order -- sequential, tree, across waves, partials,
# atomics -- puts each term through at most n - 1 roundings).  A matrix instruction that truncated internally instead
# would need about twice these c.  The count is loose: the bound does NOT catch a dropped partial product or an empty l
# plane (tests/test_head_bounds_cpu.py prints how far inside it such mutants stay).  Only the exact probes of
# tests/test_head_exact_gpu.py discriminate those; the bounds hold random inputs entry by entry, small entries included.

C_EXP = 4.0   # expf (OCML, <= 1 ulp = 2 u relative) of an exactly formed x - 1: 4 u relative to the value
C_SIG = 8.0   # 1 / (1 + expf(-x)): expf 2 u, the add and the division u each -> 4 u first order; slack x 2


def c_head_bf16x3(k: int) -> float:
    """A sum of k fp32 products (+ the bias) on the bf16 matrix pipe (tgemm, the neck / rgb / rmlp / density kernels, the
    streamed and fused weight gradients): a product a b becomes six exact bf16 x bf16 partial products; the dropped
    w_m x_l + w_l x_m + w_l x_l and the two operands' split remainders are <= 4 u |a| |b| together.  6 k partial products
    + the bias are summed in fp32: 6 k roundings.  Slack 1  ->  6 k + 5.  It also bounds the fp32 paths (k + 2 below),
    so the GPU tests use it wherever the path taken depends on the shape."""
    return float(6 * k + 5)


def c_head_fp32(k: int) -> float:
    """fp32-input MFMA (linear_fwd, the dX pass of linear_bwd, the chain kernel): bitwise a k-ordered fmaf chain, k
    roundings, the bias one more; slack 1  ->  k + 2."""
    return float(k + 2)


def _z(x):
    return None if x is None else x.double()


def head_linear(h, eh, w, b=None, extra=0):
    """z = h w^T + b and its error bound: c(k + extra) u (|h| |w|^T + |b|) + eh |w|^T.  ``extra``: further products the
    kernel sums into the same entry (e.g. a per-ray part)."""
    w = w.detach().double()
    aw = w.abs()
    z = h @ w.T
    a = h.abs() @ aw.T
    if b is not None:
        b = b.detach().double()
        z, a = z + b, a + b.abs()
    e = c_head_bf16x3(w.shape[1] + extra) * U * a
    if eh is not None:
        e = e + eh @ aw.T
    return z, e


def head_relu(z, ez, mask=None):
    """ReLU with the product's own mask (its saved activations > 0) or, without one, the fp64 mask plus the units whose
    pre-activation lies within its error bound of 0 (``amb``: either branch is correct there).  -> a, ea, mask, amb"""
    if mask is None:
        mask = z > 0
        amb = z.abs() <= ez
    else:
        mask = mask.bool()
        amb = torch.zeros_like(mask)
    return z * mask, ez * (mask | amb), mask, amb


def head_relu_bwd(d, ed, mask, amb):
    """d relu: d * mask; an ambiguous unit may take the other branch: its whole |d| is error."""
    return d * mask, ed * (mask | amb) + d.abs() * amb


def head_sigmoid(z, ez):
    y = torch.sigmoid(z)
    return y, 0.25 * ez + C_SIG * U * y.abs()


def head_sigmoid_bwd(go, y, ey):
    """go y (1 - y) from the kernel's own (inexact) y: |go| |1 - 2 y| ey, and three roundings."""
    d = go * y * (1 - y)
    return d, go.abs() * (1 - 2 * y).abs() * ey + 3 * U * d.abs()


def head_trunc_exp(f0, ef0):
    """density exp(f0 - 1) and its bound: value x error of f0, plus C_EXP u of the value (inf past fp32 stays inf)."""
    y = torch.exp(f0 - 1)
    return y, y * ef0 + C_EXP * U * y


def head_trunc_exp_bwd(gd, f0, ef0):
    """side gradient gd exp(min(f0 - 1, 15)) and its bound (exp's own error and the product's rounding; f0's error
    only below the clamp)."""
    v = torch.exp(torch.clamp(f0 - 1, max=15.0))
    s = gd * v
    return s, gd.abs() * v * (ef0 * (f0 - 1 < 15) + C_EXP * U) + U * s.abs()


def head_linear_bwd(d, ed, w, h, eh, dx_terms=None):
    """Gradients of z = h w^T + b for dz = d (error ed), h with error eh: {dW, db, dx} -> (value, bound).  dW and db sum
    over every row (c of the row count: any reduction structure); dx over the outputs (``dx_terms`` overrides the count
    when the kernel sums further products into the same entry)."""
    w = w.detach().double()
    aw = w.abs()
    M = d.shape[0]
    ad, ah = d.abs(), h.abs()
    out = {}
    ew = c_head_bf16x3(M) * U * (ad.T @ ah) + ed.T @ ah
    if eh is not None:
        ew = ew + ad.T @ eh
    out["dW"] = (d.T @ h, ew)
    out["db"] = (d.sum(0), c_head_bf16x3(M) * U * ad.sum(0) + ed.sum(0))
    out["dx"] = (d @ w, c_head_bf16x3(dx_terms or w.shape[0]) * U * (ad @ aw) + ed @ aw)
    return out


def assert_head_bound(got, ref, err, what: str, report: dict = None) -> float:
    """|got - ref| <= err entry by entry (err from the head_* propagation; err = 0 -> exactly equal)."""
    g = got.detach().double().cpu().numpy()
    r = ref.detach().double().cpu().numpy()
    e = err.detach().double().cpu().numpy()
    return assert_bound(g, r, e / U, 1.0, what, report=report)


# ------------------------------------------------------------------------------------------- proposal-loss kernel
# emer_prop_loss (csrc/proploss.hip).  Two regimes (tests/_prop_probe.py):
#
# Exact probes: everything up to the hinge argument d = max(w_s - w_p, 0) is exact, w_p = c_{j+1} - c_j too.  What follows
# are correctly rounded fp32 operations (HIP's default fp32 division is correctly rounded), counted per result below.
#
# Realistic inputs: first-order propagation through the kernel's stages (``prop_aa_bound``), one rounding per addition
# (a sum of k terms in any order puts each term through at most k - 1 roundings: it covers the kernel's chunked wave
# scans and torch's sequential cumsum alike), abs-sums from the fp64 evaluation.

C_PROP_DEN = 2.0   # den = fl(w_p + eps_f32) against w_p + eps: one rounding, and |eps_f32 - eps| <= u eps <= u den


def c_prop_term(exact_wp: bool = True) -> float:
    """One loss term d^2 / den relative to itself: d d (1), den (2, + 1 when w_p = c_{j+1} - c_j rounds), the division (1)."""
    return 1.0 + C_PROP_DEN + (0.0 if exact_wp else 1.0) + 1.0


def c_prop_G(exact_wp: bool = True) -> float:
    """G = -2 d / den - d^2 / den^2 relative to itself (both quotients have the same sign: |G| is their sum):
    q1 = fl(fl(-2 d) / den): -2 d exact, den e, the division 1                      -> (e + 1) u |q1|
    q2 = fl(fl(d d) / fl(den den)): d d 1, den den 2 e + 1, the division 1          -> (2 e + 3) u |q2|
    G = fl(q1 - q2): 1 more                                                         -> (2 e + 4) u |G|, e = 2 (3 inexact)."""
    e = C_PROP_DEN + (0.0 if exact_wp else 1.0)
    return 2.0 * e + 4.0


def c_prop_grad(exact_wp: bool = True) -> float:
    """d cdf_j = fl(fl(G_{j-1} - G_j) scale) against (|G_{j-1}| + |G_j|) scale: each G carries c_prop_G, the difference
    and the product one rounding each (relative to |G_{j-1} - G_j| <= |G_{j-1}| + |G_j|), slack 1."""
    return c_prop_G(exact_wp) + 2.0 + 1.0


def c_prop_ray_loss(k: int, exact_wp: bool = True) -> float:
    """Per-ray loss (all terms >= 0, so relative to the value itself): one term c_prop_term, ceil(k / 64) additions per
    lane, the six steps of the wave sum, the product with scale, slack 1.  k: the intervals summed (m; n in pdf mode)."""
    return c_prop_term(exact_wp) + float(-(-k // 64)) + 6.0 + 1.0 + 1.0


C_PROP_TOTAL = 1.0  # the reduction kernel accumulates in double: one final rounding (2^-53 n below the slack: |.| <= u |sum|)


def c_prop_pdf_grad(hits) -> np.ndarray:
    """Mode 1, per proposal entry, against scale sum |g| over its hits: g = fl(fl(-2 d) / den) with w exact and den
    one rounding + the constant (C_PROP_DEN) + the division (1) = 3; `hits` LDS atomics in any order (hits - 1 roundings,
    each seeing at most the abs-sum; counted hits); the product with scale (1); slack 1."""
    return np.asarray(hits, np.float64) + (C_PROP_DEN + 1.0) + 1.0 + 1.0


def _prefix(a):
    return np.cumsum(a)


def prop_aa_bound(st: dict, scale: float) -> dict:
    """First-order error bounds for mode 0 on arbitrary fp32 inputs, from the fp64 stage values ``st`` of
    tests/_prop_probe.model(..., dt=float64) for one ray.  Returns per-entry bounds for
    ``pdf``, ``cdf`` (at the knots), ``ci`` (at the proposal edges), ``ws``, ``G``, ``grad`` and ``loss``:

    * inputs: cdf_j = fl(1 - trans_j) (u |cdf_j|; cdf_n = 1 exactly), knots fl(s -+ r) (u |knot|);
    * w_n = fl(fl(dc) / fl(ds)): (e_c_j + e_c_j+1) / ds + 3 u |w_n|; events fl(fl(w_r - w_l) / 2 r): (e_wr + e_wl) / 2 r + 2 u |y|;
    * slope_t = sum of t + 1 events: t u sum |ev|, + what the events themselves carry: the two events +y_j (at knot s_j - r)
      and -y_j (at s_j + r) hold the same rounded y_j, so only the edges j_b .. j_a straddling segment t count, and their sum
      telescopes to (w_r[j_a] - w_l[j_b]) / 2 r: (e_wr[j_a] + e_wl[j_b]) / 2 r + sum over j_b .. j_a of 2 u |y_j|;
    * pdf term dx slope: e_dx |slope| + |dx| e_slope + u |term| with e_dx = e_knot_t + e_knot_t+1 + u |dx|; pdf at knot t + 1:
      sum of the term errors + t u sum |terms| (max(., 0) is 1-Lipschitz);
    * area 0.5 (p_t + p_t+1) dx: 0.5 (e_p_t + e_p_t+1 + u |p_t + p_t+1|) |dx| + 0.5 |p_t + p_t+1| e_dx + u |area|; cdf: sum + t u sum |area|;
    * CI = cdf_i0 + num (p0 + p1 off + p0 (1 - off)) / 2: e_num = e_knot_i0 + u |num|, e_off = min(1, (e_num + off e_den) / den
      + u off) (off is clipped to [0, 1]; a bracket that differs between the precisions only when q is within e_knot of a knot
      changes the value to second order: the interpolant is continuous with a continuous derivative), inner: (2 - off) e_p0
      + off e_p1 + |p1 - p0| e_off + 4 u (2 |p0| + |p1|), product and sum one rounding each;
    * w_s = fl(CI_j+1 - CI_j): the area errors of the common prefix cancel, what remains is the sum of e_area between the two
      brackets, both prefixes' additions, both interpolations; w_p = fl(c_j+1 - c_j), d = max(fl(w_s - w_p), 0): e_d = e_ws + u |w_p| + u |w_s - w_p|;
    * |dG| <= (2 / den + 2 d / den^2) e_d + c_prop_G(False) u |G| (G is continuous across the hinge: the bound holds on
      both sides), a term: (2 d / den) e_d + c_prop_term(False) u term;
    * grad_j: (e_G_j-1 + e_G_j + 2 u (|G_j-1| + |G_j|)) scale;  loss: sum of the term errors + (m + 1) u sum of terms, times scale."""
    a = lambda x: np.abs(np.asarray(x, np.float64))   # noqa: E731
    c, xr, ev = st["c"], st["xr"], st["ev"]
    K = xr.size
    e_c = U * a(c)
    e_c[-1] = 0.0
    # w_n and the events, in the order of the final edges
    dsf = np.diff(st["s"])
    e_wn = (e_c[1:] + e_c[:-1]) / dsf + 3 * U * a(st["wn"])
    e_wr, e_wl = np.append(e_wn, 0.0), np.insert(e_wn, 0, 0.0)
    # the events in knot order: position of A_j / B_j among the knots (the model's own ranks)
    e_x = U * a(xr)
    t = np.arange(K - 1, dtype=np.float64)
    # slope of segment t = sum of the events of the edges j_b .. j_a whose knots straddle it = (w_r[j_a] - w_l[j_b]) / 2 r: the
    # errors the weights carry telescope to the two outermost ones; each y_j in between adds its own two roundings
    seg = np.arange(K - 1)
    ja, jb = np.searchsorted(st["pa"], seg, "right") - 1, np.searchsorted(st["pb"], seg, "right")
    is_open = jb <= ja
    e_in = np.where(is_open, e_wr[np.maximum(ja, 0)] + e_wl[np.minimum(jb, e_wl.size - 1)], 0.0) / (2 * st["pulse"])
    y_cum = np.insert(_prefix(2 * U * a(st["y"])), 0, 0.0)
    e_own = np.where(is_open, y_cum[np.maximum(ja, 0) + 1] - y_cum[np.minimum(jb, e_wl.size - 1)], 0.0)
    e_slope = e_in + e_own + t * U * _prefix(a(ev[:K - 1]))
    dx, slope = a(st["dx"]), a(st["slope"])
    e_dx = e_x[1:] + e_x[:-1] + U * dx
    e_v = e_dx * slope + dx * e_slope + U * a(st["v"])
    e_pdf = np.insert(_prefix(e_v) + t * U * _prefix(a(st["v"])), 0, 0.0)
    psum = a(st["psum"])
    e_area = 0.5 * (e_pdf[1:] + e_pdf[:-1] + U * psum) * dx + 0.5 * psum * e_dx + U * a(st["area"])
    e_cdf_in, e_cdf_add = np.insert(_prefix(e_area), 0, 0.0), np.insert(t * U * _prefix(a(st["area"])), 0, 0.0)
    e_cdf = e_cdf_in + e_cdf_add
    i0, i1 = st["i0"], st["i1"]
    num, den, off = a(st["num"]), a(st["den"]), a(st["off"])
    p0, p1 = a(st["pdf"][i0]), a(st["pdf"][i1])
    e_num = e_x[i0] + U * num
    e_den = e_x[i0] + e_x[i1] + U * den
    with np.errstate(divide="ignore", invalid="ignore"):
        e_off = np.where(den > 0, np.minimum(1.0, (e_num + off * e_den) / den + U * off), 0.0)
    e_inner = (2.0 - off) * e_pdf[i0] + off * e_pdf[i1] + a(st["pdf"][i1] - st["pdf"][i0]) * e_off + 4 * U * (2 * p0 + p1)
    e_prod = e_num * a(st["inner"]) + num * e_inner + U * a(st["prod"])
    e_ci = e_cdf[i0] + 0.5 * e_prod + U * a(st["ci"])
    # w_s = CI_j+1 - CI_j: the area errors the two prefixes share cancel (the additions' own roundings do not)
    e_loc = e_cdf_add[i0] + 0.5 * e_prod + U * a(st["ci"])
    e_ws = a(e_cdf_in[i0][1:] - e_cdf_in[i0][:-1]) + e_loc[1:] + e_loc[:-1] + U * a(st["ws"])
    d, dn = st["d"], st["dn"]
    e_d = e_ws + U * a(st["wp"]) + U * a(st["ws"] - st["wp"])
    e_G = (2.0 / dn + 2.0 * d / dn ** 2) * e_d + c_prop_G(False) * U * a(st["G"])
    e_term = (2.0 * d / dn) * e_d + c_prop_term(False) * U * st["term"]
    gm, gj = np.insert(a(st["G"]), 0, 0.0), np.append(a(st["G"]), 0.0)
    e_grad = (np.insert(e_G, 0, 0.0) + np.append(e_G, 0.0) + 2 * U * (gm + gj)) * abs(scale)
    m = d.size
    e_loss = (e_term.sum() + (m + 1) * U * st["term"].sum()) * abs(scale)
    return dict(pdf=e_pdf, cdf=e_cdf, ci=e_ci, ws=e_ws, G=e_G, grad=e_grad, loss=e_loss)


def assert_prop_bound(got, ref, err, what: str, report: dict = None) -> float:
    """|got - ref| <= err entry by entry (numpy arrays; err = 0 -> exactly equal); prints and returns the worst err / bound."""
    return assert_bound(np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(err, np.float64) / U, 1.0, what, report=report)


def prop_pdf_bound(st: dict, scale: float) -> dict:
    """First-order bounds for mode 1 (_pdf_loss) on arbitrary fp32 inputs, from the fp64 stage values of
    tests/_prop_probe.model_pdf(..., dt=float64) for one ray: cdf_j = fl(1 - trans_j) (u |cdf_j|), w = fl(dc)
    (e_w = e_c_j + e_c_j+1 + u |w|), w_outer one rounding, d = max(fl(w - w_outer), 0): e_d = e_w + u |w_outer| + u |w - w_outer|;
    den = fl(w + eps): e_den = e_w + C_PROP_DEN u den; g = -2 d / den: (2 / den) e_d + (2 d / den^2) e_den + 2 u |g| (g is
    continuous across the hinge); an entry sums the g of the final intervals whose brackets end there -- every interval
    whose hinge is active or within e_d of it counts as a hit --: sum e_g + hits u sum |g|, + u for the product with scale.
    A term d^2 / den: (2 d / den) e_d + (d^2 / den^2) e_den + 3 u term; the loss over n terms: + (n + 1) u sum."""
    a = lambda x: np.abs(np.asarray(x, np.float64))   # noqa: E731
    c, w, wo, d, dn, g = st["c"], st["w"], st["wo"], st["d"], st["dn"], st["g"]
    e_c = U * a(c)
    e_c[-1] = 0.0
    e_w = e_c[1:] + e_c[:-1] + U * a(w)
    e_d = e_w + U * a(wo) + U * a(w - wo)
    e_den = e_w + C_PROP_DEN * U * dn
    e_g = (2.0 / dn) * e_d + (2.0 * d / dn ** 2) * e_den + 2 * U * a(g)
    pot = (w - wo) > -e_d
    m1 = st["G"].size
    e_sum, hits, gabs = np.zeros(m1), np.zeros(m1), np.zeros(m1)
    for idx in (st["ir"], st["il"]):
        np.add.at(e_sum, idx[pot], e_g[pot])
        np.add.at(hits, idx[pot], 1.0)
        np.add.at(gabs, idx[pot], a(g)[pot])
    e_grad = (e_sum + (hits + 1.0) * U * gabs) * abs(scale)
    e_term = (2.0 * d / dn) * e_d + (d * d / dn ** 2) * e_den + 3 * U * st["term"]
    e_loss = (e_term.sum() + (d.size + 1) * U * st["term"].sum()) * abs(scale)
    return dict(grad=e_grad, loss=e_loss)


# ------------------------------------------------------------------------------------------- compositing kernels
# csrc/composite.hip and the ray epilogue of csrc/rayloss.hip on arbitrary fp32 inputs (tests/_composite_probe.py has the
# fp64 restatement whose values and abs-sums these take).  First order, one rounding (relative u) per fp32 operation; a
# contracted multiply-add only removes roundings.  A sum of terms through any tree puts each term through at most
# `depth` additions, each seeing a partial sum that is at most the abs-sum: depth u abs_sum.
#
# The one constant that is not derived is the device expf's error.  Measured on an MI355X through render_weights_fwd itself
# (S = 2, dt = 1, sigma_1 = 0: trans[:, 1] = expf(-sigma_0)), 11.5 million arguments in [0, 100] (a uniform grid, uniform
# random, dense in [0, 2], log-spaced down to e^-30, every multiple of 0.25) against float64 exp of the fp32 argument:
# at most 0.836 ulp (at x = 62.4916; 6.3 % of the results are not the correctly rounded one), results below the normal range
# are kept and within one subnormal step.  E_EXPF is that maximum rounded up to the next integer plus one ulp of margin;
# one ulp is at most 2 u relative.  tests/test_composite_exact_gpu.py::test_device_expf_error_is_inside_E_EXPF repeats a
# smaller sweep and fails if the device's expf ever leaves E_EXPF - 1.
E_EXPF_MEASURED = 0.836  # ulps
E_EXPF = 2.0
TINY = 2.0 ** -126       # absolute floor: results below the normal range (kept or flushed)


def _chunk(S):
    return np.arange(S) // 64


def render_bounds(rf: dict) -> dict:
    """render_weights_fwd / composite_rgb_fwd from ``ref_render``'s values (x = sigma dt, A = inclusive cumsum |x|):

    * x = fl(sigma fl(te - ts)): 2 u |x|;
    * excl_i: every x_j passes the 6 steps of the wave scan, `incl - sdt`, `carry +` and one carry accumulation per earlier
      chunk c_i: depth 8 + c_i, partial sums at most A_i; what the x_j carry themselves: 2 u A_i  ->  (10 + c_i) u A_i;
    * T = expf(-excl): the ABSOLUTE error of excl becomes a RELATIVE error of T: expm1(e_excl) + 2 E_EXPF u;
    * e = expf(-x): (expm1(e_x) + 2 E_EXPF u) e; alpha = fl(1 - e): e_e + u alpha -- absolute, u-sized even where alpha is tiny;
    * w = fl(T alpha): T e_alpha + alpha e_T + u w;  cdfs = fl(1 - T): e_T + u |1 - T| (the last column is written as 1);
    * sum w, sum w mid: each lane adds one w per chunk, then the 6 steps of the wave sum: depth n_chunks + 6; mid = fl(fl(a + b) / 2)
      and the product: 2 u w mid;
    * the median's inclusive cumsum of w: 6 scan steps, `wcarry +`, one carry per earlier chunk: (7 + c_i) u cumsum(w) + cumsum(e_w).
    """
    x, A, T, e, al, w, mid = (rf[k] for k in ("x", "A", "T", "e", "al", "w", "mid"))
    S = x.shape[1]
    c = _chunk(S)[None, :]
    nch = -(-S // 64)
    e_x = 2 * U * np.abs(x)
    e_excl = (10 + c) * U * A
    rel = 2 * E_EXPF * U
    r_T = np.expm1(e_excl)
    e_T = T * (r_T + rel * (1 + r_T)) + TINY
    r_e = np.expm1(e_x)
    e_e = e * (r_e + rel * (1 + r_e)) + TINY
    e_al = e_e + U * np.abs(al)
    e_w = T * e_al + al * e_T + e_T * e_al + U * w + TINY
    e_cdf = np.concatenate([e_T + U * np.abs(1 - T), np.zeros((x.shape[0], 1))], 1)
    e_sum = e_w.sum(1) + (nch + 6) * U * w.sum(1)
    e_mid = (e_w * mid + 2 * U * w * mid).sum(1) + (nch + 6) * U * (w * mid).sum(1)
    e_cw = np.cumsum(e_w, 1) + (7 + c) * U * np.cumsum(w, 1)
    return dict(x=e_x, T=e_T, e=e_e, al=e_al, w=e_w, cdfs=e_cdf, wsum=e_sum, wmid=e_mid, cw=e_cw,
                weights=e_w, trans=e_T, alphas=e_al)


def median_ambiguous(rf: dict, rb: dict) -> np.ndarray:
    """Rays whose fp64 inclusive cumsum of w comes within its bound of 0.5 at some sample: the median may slip there."""
    return (np.abs(rf["cw"] - 0.5) <= rb["cw"]).any(1)


def dsigma_bound(rf: dict, rb: dict, g: dict) -> np.ndarray:
    """d_sigma_i = fl(dt (gw T e - later + gA e)) of render_weights_bwd / composite_rgb_bwd.  ``g`` (``ref_render_bwd`` plus
    gw_abs, gT_abs and the per-ray errors e_g0, e_g1 that reach gw):

    * gw = dW [+ sum_c g_c rgb_c] + (g0 + g1 mid): at most 6 roundings on the abs-sum gw_abs, plus e_g0 + e_g1 mid;
    * P = gw T e: e_gw T e + |gw| (e_T e + T e_e) + 2 u |P|;
    * term_k = gw_k w_k + gT_k T_k: e_gw w + |gw| e_w + |gT| e_T + 4 u (|gw| w + gT_abs T) (two products, one sum, and the
      wrapper's fp32 sum dT - dC);
    * later_i = suffix + (sfx_incl - term): 6 scan steps, the subtraction, `suffix +`, one carry per later chunk: depth
      8 + (n_chunks - 1 - c_i) on the INCLUSIVE abs-sum of the terms from i on -- `sfx_incl - term` cancels, so it is held to
      the abs-sum, never to the result;
    * Q = gA e: |gA| e_e + u |Q|;
    * `P - later + Q` and the product with dt = fl(te - ts): 4 u on |P| + abs-sum + |Q|, again not on the result."""
    T, e, w, mid, dts = (rf[k] for k in ("T", "e", "w", "mid", "dts"))
    S = T.shape[1]
    c = _chunk(S)[None, :]
    nch = -(-S // 64)
    a = np.abs
    gw, gT, gA = g["gw"], g["gT"], g["gA"]
    e_gw = 6 * U * g["gw_abs"] + g["e_g0"][:, None] + g["e_g1"][:, None] * mid
    e_P = e_gw * T * e + a(gw) * (rb["T"] * e + T * rb["e"] + rb["T"] * rb["e"]) + 2 * U * a(g["P"])
    t_abs = (a(gw) + e_gw) * w + g["gT_abs"] * T
    e_term = e_gw * (w + rb["w"]) + a(gw) * rb["w"] + a(gT) * rb["T"] + 4 * U * t_abs
    rc = lambda v: np.cumsum(v[:, ::-1], 1)[:, ::-1]   # noqa: E731
    L_abs = rc(t_abs)
    e_L = np.concatenate([rc(e_term)[:, 1:], np.zeros_like(T[:, :1])], 1) + (8 + nch - 1 - c) * U * L_abs
    e_Q = a(gA) * rb["e"] + U * a(g["Q"])
    return a(dts) * (e_P + e_L + e_Q + 4 * U * (a(g["P"]) + L_abs + a(g["Q"])))


C_EPI_GO = 8.0   # go = do - gd y / (o o) - sum_c g_c sky_c: a term's own roundings (<= 3) + 4 subtractions, slack 1


def epilogue_bounds(ep: dict, e_sum=None, e_mid=None, e_acc=None) -> dict:
    """ray_epilogue_fwd/bwd and the per-ray part of composite_rgb from ``ref_epilogue``'s values.  e_sum / e_mid / e_acc: the
    errors the inputs (sum w, sum w mid, accumulated colour) already carry -- 0 when the kernel is given them exactly.

    * opacity = clamp(sum w): exact given its input; e_o = e_sum where the clamp passes (or may pass), else 0;
    * depth = fl(y / o): e_mid / o + |y| e_o / o^2 + u |depth|;
    * rgb = fl(acc + fl(sky fl(1 - o))): e_acc + |sky| e_o + 2 u |sky (1 - o)| + u (|acc| + |sky (1 - o)|);
    * g1 = fl(gd / o): |gd| e_o / o^2 + u |g1|;  d_sky = fl(g fl(1 - o)): |g| e_o + 2 u |g (1 - o)|;
    * g0: C_EPI_GO u on the abs-sum of go, plus |gd| (e_mid / o^2 + 2 |y| e_o / o^3), on the rays of ``ep["passes"]``; exactly
      0 on the others.  The caller evaluates the reference with the clamp branch the kernel took
      (tests/_composite_probe.clamp_branch), so a ray whose sum w sits on a clamp bound gets no allowance."""
    a = np.abs
    o, st = ep["opacity"], ep["stats"]
    R = o.shape[0]
    z = np.zeros(R)
    e_sum, e_mid = (z if e_sum is None else e_sum), (z if e_mid is None else e_mid)
    lo = float(np.float32(1e-6))
    inside = (st[:, 0] >= lo - e_sum) & (st[:, 0] <= 1.0 + e_sum)
    e_o = np.where(inside, e_sum, 0.0)
    y = st[:, 1]
    out = dict(opacity=e_o, depth=e_mid / o + a(y) * e_o / o ** 2 + U * a(ep["depth"]))
    if "rgb" in ep:
        e_acc = np.zeros_like(ep["rgb"]) if e_acc is None else e_acc
        sk = ep["rgb"] - ep["acc"]           # sky (1 - o), or 0 without a sky
        sky_abs = np.zeros_like(sk) if ep.get("sky") is None else a(ep["sky"])
        out["rgb"] = e_acc + sky_abs * e_o[:, None] + 2 * U * a(sk) + U * (a(ep["acc"]) + a(sk))
    if "d_sky" in ep:
        out["d_sky"] = ep["g_abs"] * e_o[:, None] + 2 * U * a(ep["d_sky"])
    dd = ep["dd"]
    out["g1"] = a(dd) * e_o / o ** 2 + U * a(ep["g1"])
    e_go = C_EPI_GO * U * ep["go_abs"] + a(dd) * (e_mid / o ** 2 + 2 * a(y) * e_o / o ** 3)
    out["g0"] = np.where(ep["passes"], e_go, 0.0)
    return out


def c_accumulate(S: int, C) -> float:
    """out[r, c] = sum_s w v against sum |w v|: small kernel (C <= 8 or no values): the product, ceil(S / 64) additions per
    lane, 6 wave-sum steps; wide kernel: the product and S sequential additions.  Slack 1."""
    return float(-(-S // 64) + 8) if (C is None or C <= 8) else float(S + 2)


def c_accumulate_dw(C) -> float:
    """d_w = sum_c go v against sum |go v|: small: C products, C - 1 additions; wide: product, ceil(C / 64) additions per
    lane, 6 wave-sum steps.  Slack 1.  (No values: d_w is go itself, exactly.)"""
    return float(C + 1) if C <= 8 else float(-(-C // 64) + 8)


def blend_c(S: int, wide_C=None) -> dict:
    """Rounding counts of blend_accumulate (wide_C None) and blend_accumulate_wide against the abs-sums of
    ``ref_blend`` / ``ref_blend_wide``; slack 1 in each.  inv = fl(1 / fl(sigma + 1e-6f)): 2; a = sigma_s inv: 3;
    ka = a fl(1 - shadow): 5.

    narrow: a forward term w (ka rgb_s + b rgb_d): 8, the lane's chain ceil(S / 64), the wave sum 6; sum w shadow^2: 2 + chain;
      <g, rgb>: 3; d_w = ka gS + b gD + gs sh sh: 11; d_rgb_s = g (w ka): 7; d_rgb_d = g (w b): 5; d_shadow = w (2 gs sh - a gS): 9;
      d_sigma_s = (w (1 - sh) gS) inv: 9; d_sigma_d = (w gD) inv: 7; d_sigma = -(da sigma_s + db sigma_d) inv inv: 14.
    wide: a forward term w (a f_s + b f_d): 6, a chain of ceil(S / 8) + 1 per wave, a0 + a1 and two cross-wave additions: 3;
      m = <g, f>: cm = the product, ceil(C / 64) per lane, 6 wave-sum steps; d_w = a mS + b mD: cm + 5; d_f = g (w sigma inv): 5;
      d_sigma_s = (w mS) inv: cm + 4; d_sigma = ...: cm + 9."""
    if wide_C is None:
        ch = -(-S // 64)
        return dict(acc=15.0 + ch, acs=9.0 + ch, d_w=12.0, d_rs=8.0, d_rd=6.0, d_sh=10.0, d_ss=10.0, d_sd=8.0, d_sig=15.0)
    cm = -(-wide_C // 64) + 7
    return dict(acc=float(-(-S // 8) + 11), d_w=cm + 6.0, d_fs=6.0, d_fd=6.0, d_ss=cm + 5.0, d_sd=cm + 5.0, d_sig=cm + 10.0)


def assert_err_bound(got, ref, err, what: str, report: dict = None) -> float:
    """|got - ref| <= err entry by entry (numpy; err = 0 -> exactly equal); prints and returns the worst err / bound."""
    ref = np.asarray(ref, np.float64)
    return assert_bound(np.asarray(got, np.float64).reshape(ref.shape), ref, np.broadcast_to(np.asarray(err, np.float64), ref.shape) / U, 1.0,
                        what, report=report)


# ------------------------------------------------------------------------------------------------------ loss kernels
# pixel_loss, lidar_loss and reg_losses of csrc/rayloss.hip on arbitrary fp32 inputs (tests/_loss_probe.py has the fp64
# restatements whose values these take).  First order, one rounding (relative u) per fp32 operation, a host float that
# arrives as a c_float counted as one; a contracted multiply-add only removes roundings.
#
# The one constant that is not derived is the device logf's error.  Measured on an MI355X through pixel_loss_fwd itself
# (sky-only, w_sky = 1, R = 2^23, so that loss_rays[r] = -logf(arg_r) / R exactly) on the 8 388 608 opacities of
# tests/test_loss_exact_gpu._logf_sweep(23) in [1e-6, 1]: 2^21 log-spaced from 1e-6, 2^21 of 1 - log-spaced down to 1 - 1e-7,
# 2^20 each of uniform random, dense random in [1e-6, 1e-3], dense random in [0.999, 1] and a uniform grid; once with
# sky_mask = 0 for logf(o) and once with sky_mask = 1 for logf(fl(1 - o)), against float64 log of the fp32 argument: at most
# 2.140 ulp for logf(o) (at o = 1.4565692e-05) and 2.143 ulp for logf(1 - o) (at 1 - o = 0.061523914); 48 % of the results are
# not the correctly rounded one; about 2.1 ulp throughout (0, 0.5] and 1.9 ulp in (0.5, 1); logf(1) = 0 and logf(0) = -inf
# (clamped to -100) exactly.  E_LOGF is the measured maximum rounded up to the next integer plus one ulp of margin (the rule
# E_EXPF follows); one ulp is at most 2 u relative.  test_device_logf_error_is_inside_E_LOGF runs _logf_sweep(20), the same
# generator at 2^20 arguments, in the suite and fails if the device's logf ever leaves E_LOGF - 1.
E_LOGF_MEASURED = 2.143  # ulps
E_LOGF = 4.0

C_PIX_RGB = 10.0   # w s / (3 R): d = fl(a - b) squared 3, the sum of three 2, the c_float w, the product, fl(3 R), the division 4; slack 1
C_PIX_DRGB = 7.0   # up w 2 d / (3 R): the c_float w gs, up w, d, the product, fl(3 R), the division; slack 1
C_PIX_DOPA = 9.0   # up w (o - t) / max(o fl(1 - o), 1e-12f) / R: w gs, up w, o - t, the product, 1 - o, o (1 - o), two divisions; slack 1


def pixel_bounds(st: dict) -> dict:
    """Per-ray pixel loss and its two gradients from ``restate_pixel``'s values.

    * rgb term: C_PIX_RGB u |term|;
    * BCE = -(t max(logf(o), -100) + (1 - t) max(logf(fl(1 - o)), -100)): logf carries 2 E_LOGF u |log|; fl(1 - o) carries a
      relative u, which is an ABSOLUTE -log1p(-u) in its logarithm (near o = 1 the term log(1 - o) sees the absolute rounding of
      1 - o); a clamped logarithm is exact; the two products and the sum: u (|A| + |B|) + u |A + B|; w bce / R: the c_float w, the
      product and the division, 3 u;
    * the sum of the two terms: u |ray|;  the gradients: C_PIX_DRGB / C_PIX_DOPA u |value| (the floor 1e-12f is the same constant
      in the restatement, and o (1 - o) is never near it for o in [1e-6, 1] unless it is exactly 0)."""
    a = np.abs
    R = st["R"]
    e_sky = np.zeros(R)
    if "o" in st:
        t = st["t"]
        lo, l1 = np.maximum(st["log_o"], -100.0), np.maximum(st["log_1mo"], -100.0)
        rel = 2 * E_LOGF * U
        r1 = -np.log1p(-U)
        e_lo = np.where(st["log_o"] > -100.0, rel * a(lo), 0.0)
        e_l1 = np.where(st["log_1mo"] > -100.0, r1 + rel * (a(l1) + r1), 0.0)
        e_bce = a(t) * e_lo + a(1 - t) * e_l1 + U * (a(st["A"]) + a(st["B"])) + U * a(st["A"] + st["B"])
        e_sky = a(st["w_sky"]) / R * e_bce + 3 * U * a(st["sky_term"])
    out = dict(rays=C_PIX_RGB * U * a(st["rgb_term"]) + e_sky + U * a(st["rays"]))
    if st.get("d_rgb") is not None:
        out["d_rgb"] = C_PIX_DRGB * U * a(st["d_rgb"])
    if st.get("d_opa") is not None:
        out["d_opa"] = C_PIX_DOPA * U * a(st["d_opa"])
    return out


C_LIDAR_SCALE = 4.0   # scale = w_sight fl(n_pos / R) / R: the c_float w_sight, two divisions, one product
C_LIDAR_NORM = 6.0    # norm = 1 / sqrtf(2 pi_f sigma sigma), sigma = fl(fl(eps) / 3): pi_f 1, sigma 2 twice, two products 2 -> 7 u under
#                       the root = 3.5 u, the root 1, the division 1: 5.5 u against 1 / sqrt(2 pi (eps / 3)^2) in double
C_LIDAR_INV2S2 = 6.0  # inv2s2 = 1 / (2 sigma sigma): sigma 2 twice, one product, the division


def lidar_bounds(st: dict, eps: float) -> dict:
    """Per-ray lidar loss, d_depth and d_weights from ``restate_lidar``'s values.

    * x = fl(t - gt): u |x|; the argument a = fl(fl(x x) inv2s2): (2 + 1 + C_LIDAR_INV2S2 + 1) u a -- an ABSOLUTE error of the
      argument, which is a RELATIVE error expm1(e_a) of expf (a <= 4.5 in the band: inside the range E_EXPF was swept over);
      delta = fl(norm expf(-a)): (expm1(e_a) + 2 E_EXPF u + (C_LIDAR_NORM + 1) u) delta;
    * e = fl(w - delta): e_delta + u (|w| + |delta|) -- held to |w| + |delta|, not to |e|; term = e e: 2 |e| e_e + u e^2; an empty-band
      term w w: u w^2; a sample in neither band: exactly 0;
    * the wave sum: every term passes at most ceil(S / 64) + 6 additions: that many u on the abs-sum (the terms are non-negative);
    * d_w = fl(fl(up scale) dw): |up scale| 2 e_e + (C_LIDAR_SCALE + 2) u |up scale| 2 (|w| + |delta|) (empty band: 2 |w|);
    * depth: pn, gn one division each, d = fl(pc - gn): u (|pc| + |gn| + |d|); w_depth d d / n_valid: 2 |d| e_d w / n + 4 u |l|;
      d_depth = up w 2 d / (max n): |.| e_d / |d| ... + 5 u |value|; exactly 0 on an invalid ray and where the clamp blocks;
    * loss_rays = fl(l + fl(scale acc)): + (C_LIDAR_SCALE + 1) u on the sight share, + u |ray|."""
    a = np.abs
    S = st["S"]
    w, delta, e, arg, x = st["w"], st["delta"], st["e"], st["arg"], st["x"]
    near, empty = st["near"], st["empty"]
    e_a = (4 + C_LIDAR_INV2S2) * U * arg
    r_d = np.expm1(e_a)
    e_delta = delta * (r_d + (2 * E_EXPF + C_LIDAR_NORM + 1) * U * (1 + r_d)) + TINY
    e_e = e_delta + U * (a(w) + delta)
    e_term = np.where(empty, U * w * w, np.where(near, 2 * a(e) * e_e + e_e ** 2 + U * e * e, 0.0))
    dw_abs = np.where(empty, 2 * a(w), np.where(near, 2 * (a(w) + delta), 0.0))
    k = abs(st["up"] * st["scale"])
    e_dw = k * np.where(near, 2 * e_e, 0.0) + (C_LIDAR_SCALE + 2) * U * k * dw_abs
    term = st["term"]
    e_acc = e_term.sum(1) + (-(-S // 64) + 6) * U * term.sum(1)
    sc = abs(st["scale"])
    nv = max(st["n_valid"], 1)
    d, wd, mx = st["d"], abs(st["w_depth"]), st["max_depth"]
    e_d = U * (a(st["pc"]) + a(st["gn"]) + a(d))
    e_ld = np.where(st["valid"], 2 * a(d) * e_d * wd / nv + 4 * U * a(st["ray_depth"]), 0.0)
    e_dd = np.where(st["valid"] & st["passes"], abs(st["up"]) * wd * 2 * e_d / (mx * nv) + 5 * U * a(st["d_depth"]), 0.0)
    e_rays = e_ld + sc * e_acc + (C_LIDAR_SCALE + 1) * U * sc * term.sum(1) + U * a(st["rays"])
    return dict(rays=e_rays, d_depth=e_dd, d_w=e_dw)


C_REG_GRAD_CONST = 5.0   # up gs (c / n): the c_float gs and c, up gs, c / n, the product; slack 0
C_REG_GRAD = 8.0         # g (a - b) with g = up gs (2 c / n): 5 as above, the difference / sum of two fp32 inputs, the product; slack 1


def reg_partial_bound(name: str, n: int, stride: int) -> float:
    """Roundings a term of a reg_losses block partial passes, against (c / n) sum |term| over the block's elements: the
    per-thread strided chain ceil(n / stride), the 6 steps of the wave butterfly, the 4 wave partials, the c_float c, c / n and
    the product 3, the `l +=` of up to four terms 3, and the term's own: 0 (dyn, shadow), 3 ((a - b)^2), 8 (u u + v v with u, v
    sums held to the squares' own size: 3 each, the sum 1, slack 1)."""
    own = {"dyn": 0.0, "shadow": 0.0, "feat": 3.0, "cycle": 8.0}[name]
    return float(-(-n // stride) + 6 + 4 + 3 + 3) + own


# ------------------------------------------------------------------------------------------- per-ray head kernels
# csrc/rayinputs.hip on arbitrary fp32 inputs: fp32 fmaf chains, the fp32-input MFMA and float atomics, held per entry to
# c u abs_sum with abs_sum = sum |a| |b| + |bias| + |preloaded target| (every rounding sees a partial sum of at most that).
# One rounding per addition, as for the MLP heads above; c counts the additions a term can pass through, slack 1 each.
# tests/test_ray_exact_gpu.py holds the same kernels bit for bit on grid operands; these bounds hold random data entry by
# entry, small entries included.  Worst err / bound on an MI355X (test_ray_pre_matches_fp64, test_ray_wgrad_matches_fp64 and
# test_ray_inputs_and_embedding_gradient of tests/test_kernels_gpu.py at their shapes): ray_pre_fwd 0.28 (R = 70, Kh = 7), ray_pre_bwd
# 0.098, ray_wgrad 0.022 (M = 1; 0.003 at M = 8192), embed_grad 0.042 (R = 8192, n_emb = 150); torch's fp32 evaluation on the CPU:
# 0.34, 0.055, 0.046, 0.018 (tests/test_ray_bounds_cpu.py).


def c_ray_pre_fwd(kh: int) -> float:
    """ray_pre_fwd: per output an fmaf chain over k = 0 .. kh-1 that starts from the bias: kh roundings; slack 1."""
    return float(kh + 1)


def c_ray_pre_bwd(n_hidden: int) -> float:
    """ray_pre_bwd: an fmaf chain over the 2 H columns of [s0 | s1] from zero: 2 H roundings; slack 1."""
    return float(2 * n_hidden + 1)


def c_ray_wgrad(m: int) -> float:
    """ray_wgrad: a wave accumulates 64 rows of a 256-row chunk (2 rounds x 8 MFMA steps x 4 rows; one rounding per row
    counted, however the instruction rounds its four products inside) = 64; the three quarter folds, of which a term passes
    through at most two (2 + 0 / 3 + 1, then 0 + 1) = 2; one float atomic per chunk onto the target, each seeing the whole
    partial = ceil(m / 256), the target's own value included in abs_sum; slack 1."""
    return float(64 + 2 + -(-m // 256) + 1)


def c_embed_grad(n_rays: int) -> float:
    """embed_grad: a lane adds list entries two at a time, (ga + gb) + (ga' + gb') then acc += : 3 roundings for a term's own
    iteration and one for each later iteration of at most 4 per scan round of 8192 rays (512 list slots / 128 per iteration)
    = 4 ceil(R / 8192) + 2; six butterfly steps 6; the fixed-order sum over sixteen waves 16; the add onto the target 1;
    slack 1."""
    return float(4 * -(-n_rays // 8192) + 2 + 6 + 16 + 1 + 1)


# The one constant that is not derived is the device sinf's error in the sin columns of the direction rows (emer_dir_encode,
# emer_ray_inputs_fwd: sinf(x 2^k) and sinf(fl(x 2^k + half_pi_f32))).  Measured on an MI355X through emer_dir_encode itself
# (remap off, max_deg = 1: the twelve sin columns of a row are sinf of a, 2 a, fl(a + hp), fl(2 a + hp) for its three
# components) on the 38 348 616 arguments that tests/_ray_probe.sinf_sweep(21) yields -- |arg| up to 2053.6, twice what
# max_deg = 10 forms from |x| <= 1, both signs: 2^21 uniform in [-1026, 1026], 2^21 uniform in [-2, 2], 2^20 log-spaced
# magnitudes from 2^-40, the +-1600 fp32 neighbours of every zero crossing k pi and every eighth neighbour of every extremum
# up to 326 pi, the 2^-10 grid times 2^k, 2^21 of x 2^k for uniform x -- against float64 sin of the fp32 argument: at most
# 1.572 ulp of the result (at 1061.6062; 14.9 % of the results are not the correctly rounded one; by |arg|: 1.05 ulp below 2,
# 1.44 in [2, 8), 1.52 in [8, 64), 1.55 in [64, 300), 1.57 beyond).  The error IS result-relative at the zero crossings: 1.18
# ulp of the result over the 159 739 arguments within 1e-3 of a crossing k pi, k != 0 (results down to 2^-20), 0.48 ulp for
# results in [2^-40, 2^-20), exact below (sinf(x) = x) and sinf(0) = 0: the argument reduction keeps enough bits of pi, so NO
# absolute term is added.  E_SINF is the smallest power of two that is at least 1.5 x the measured maximum (1.5 x 1.572 =
# 2.36 -> 4).  tests/test_ray_exact_gpu.py::test_device_sinf_error_is_inside_E_SINF runs sinf_sweep(17) in the suite.
E_SINF_MEASURED = 1.572  # ulps
E_SINF = 4.0


# ------------------------------------------------------------------------------- update kernels of csrc/elementwise.hip
# emer_adam_step, emer_contract_bwd and emer_flow_warp_bwd on arbitrary fp32 inputs (tests/_update_probe.py has the fp64
# restatements whose intermediates these take).  Running-error bounds to first order: every fp32 operation adds u times the
# size of its own result to the error its operands already carry, and that error travels on through the derivative of the
# next operation.  The file forbids FMA contraction (every product and sum rounds on its own), and the project's compiler
# flags (-O3, no fast-math option, no option that relaxes division or square root: emernerf_amd/_build.py) leave the
# division and sqrtf correctly rounded, so every operation costs exactly one u and NOTHING here is measured.  Hyperparameters
# enter the restatement as the c_float values the ABI receives and so carry no error of their own; the two bias corrections
# are formed in double on the host and narrowed to float: one u each.  Where a denominator or a root's argument carries an
# error the rigorous form is used instead of the derivative (a / (b - e_b), e / (sqrt x + sqrt(x - e))): it equals the
# first-order term when the error is small and stays an upper bound when a cancellation in g gs + wd p made it large.
UPDATE_SLACK = 1.5       # second-order terms of the remaining products, and the fp64 restatement's own roundings
UPDATE_FLOOR = 2.0 ** -149   # a product or quotient that leaves the normal range rounds to this grid instead of to u |x|


def _r(x):
    """The rounding of one fp32 operation whose exact result is x (an exact zero stays exact)."""
    return U * np.abs(x) + np.where(np.asarray(x) != 0, UPDATE_FLOOR, 0.0)


def adam_bounds(st: dict) -> dict:
    """Absolute bounds on m', v', p' of one emer_adam_step from ``restate_adam``'s intermediates.  In the kernel's order:

    * gi = fl(g gs) [1; exact for gs = 1], + fl(wd p) [1] and the sum [1] when wd != 0;
    * m' = m + fl(fl(gi - m) fl(1 - b1)): the difference 1, fl(1 - b1) 1 and the product 1 (3 u on the product, the
      difference's share through the factor 1 - b1), the sum 1;
    * v' = fl(v b2) + fl(fl(fl(1 - b2) gi) gi): v b2 1; fl(1 - b2) and two products 3, the error of gi twice (2 |gi| e + e^2);
      the sum 1;
    * s = sqrtf(v'): e_v / (sqrt v' + sqrt(v' - e_v)) + u s  (= e_v / (2 sqrt v') to first order);
    * denom = fl(s / bc2_sqrt) + eps: the narrowed bc2_sqrt 1 and the division 1, the sum 1;
    * r = fl(m' / denom): (e_m + |r| e_denom) / (denom - e_denom) + u |r|;
    * p' = p - fl(step_size r), step_size = fl(lr / fl(bc1)): the narrowed bc1, the division and the product 3, the
      difference 1."""
    a = np.abs
    c = st["c"]
    e_gi = np.zeros_like(st["gi"]) if c["gs"] == 1.0 else _r(st["g_gs"])
    if c["wd"] != 0.0:
        e_gi = e_gi + _r(st["wd_p"]) + _r(st["gi"])
    omb1, omb2 = 1.0 - c["b1"], 1.0 - c["b2"]
    e_m = omb1 * (e_gi + _r(st["d"])) + 2 * _r(st["d"] * omb1) + _r(st["m1"])
    e_v = _r(st["v_b2"]) + omb2 * (2 * a(st["gi"]) * e_gi + e_gi ** 2) + 3 * _r(st["g2"]) + _r(st["v1"])
    s = st["s"]
    e_s = e_v / np.maximum(s + np.sqrt(np.maximum(st["v1"] - e_v, 0.0)), 1e-300) + _r(s)
    e_s = np.where(e_v == 0.0, _r(s), e_s)
    e_den = e_s / c["bc2_sqrt"] + 2 * _r(st["s_bc"]) + _r(st["denom"])
    lo = st["denom"] - e_den
    assert (lo > 0).all(), "adam_bounds: a denominator's error reaches its size"
    e_r = (e_m + a(st["r"]) * e_den) / lo + _r(st["r"])
    e_p = c["step_size"] * e_r + 3 * _r(st["upd"]) + _r(st["p1"])
    return dict(m=UPDATE_SLACK * e_m, v=UPDATE_SLACK * e_v, p=UPDATE_SLACK * e_p)


def contract_bwd_bounds(st: dict) -> np.ndarray:
    """Absolute bound [n, 3] on emer_contract_bwd's gradient from ``restate_contract_bwd``'s intermediates; st["e_p"] /
    st["e_g"] are errors the position / the incoming gradient already carry (0 for the kernel's own inputs).  A point the fp32
    forward puts outside has the bound 0: its gradient is exactly 0.

    * bounded, and unbounded with mag < 1 (out = g / w, resp. fl(fl(g / 4) 2) / w: the power-of-two steps are exact): the
      width fl(hi - lo) 1 and the division 1 -> 2 u |out| + e_g's share;
    * unbounded, mag >= 1:  a = fl(p - lo) 1;  b = fl(a / w) 2;  u = fl(2 b - 1) 1 (2 b exact) -> e_u = 2 e_b + u |u|;
      mag = |u_k|;  inv = fl(1 / mag): e_mag / (mag (mag - e_mag)) + u inv;
      f = fl(2 inv - fl(inv inv)): 2 e_inv + (2 inv e_inv + u inv^2) + u |f|;
      df = fl(fl(-2 inv inv) + fl(fl(2 inv inv) inv)): 4 inv e_inv + u |A|, 6 inv^2 e_inv + 2 u |B|, the sum 1;
      dotug = (t_0 + t_1) + t_2 with t_d = fl(u_d g_d / 4): |g_d / 4| e_u + |u_d| e_g / 4 + u |t_d| each, two sums <= 2 u sum |t_d|;
      term = fl(sgn df dotug): |dotug| e_df + |df| e_dot + e_df e_dot + u |term|;
      gu_d = fl(f g_d / 4) [|g_d / 4| e_f + |f| e_g / 4 + u] (+ term on axis k: e_term + u |gu_k|);
      out_d = fl(2 gu_d / w_d): the width 1, the division 1."""
    a = np.abs
    w, out = a(st["w"])[None, :], st["out"]
    e_g = np.broadcast_to(np.asarray(st.get("e_g", 0.0), np.float64), out.shape)
    inside = st["inside"][:, None]
    if not st["unbounded"]:
        return np.where(inside, UPDATE_SLACK * (e_g / w + 2 * _r(out)), 0.0)
    ge1 = st["ge1"]
    e_p = np.broadcast_to(np.asarray(st.get("e_p", 0.0), np.float64), out.shape)
    e_a = e_p + _r(st["a"])
    e_b = e_a / w + 2 * _r(st["b"])
    e_u = 2 * e_b + _r(st["u"])
    k = st["k"][:, None]
    e_mag = np.take_along_axis(e_u, k, 1)[:, 0]
    mag, inv, f, df = st["mag"], st["inv"], st["f"], st["df"]
    assert (e_mag[ge1] < 0.5 * mag[ge1]).all(), "contract_bwd_bounds: the error of mag reaches its size"
    e_inv = e_mag / (mag * (mag - e_mag)) + _r(inv)
    e_f = 2 * e_inv + 2 * inv * e_inv + _r(inv * inv) + _r(f)
    e_df = 4 * inv * e_inv + _r(2 * inv * inv) + 6 * inv * inv * e_inv + 2 * _r(2 * inv ** 3) + _r(df)
    g4, e_g4 = st["g4"], e_g / 4
    t = st["t"]
    e_dot = (a(g4) * e_u + a(st["u"]) * e_g4 + e_u * e_g4 + _r(t)).sum(1) + 2 * U * a(t).sum(1)
    dot = st["dot"]
    e_term = a(dot) * e_df + a(df) * e_dot + e_df * e_dot + _r(st["term"])
    fg = f[:, None] * g4
    e_gu = a(g4) * e_f[:, None] + a(f)[:, None] * e_g4 + e_f[:, None] * e_g4 + _r(fg)
    onk = np.arange(3)[None, :] == k
    e_gu = e_gu + np.where(onk, e_term[:, None] + _r(st["gu"]), 0.0)
    e_gu = np.where(ge1[:, None], e_gu, e_g4)
    e_out = 2 * e_gu / w + 2 * _r(out)
    return np.where(inside, UPDATE_SLACK * e_out, 0.0)


def flow_warp_bwd_bounds(st: dict) -> np.ndarray:
    """Absolute bound [n, 6] on emer_flow_warp_bwd's dflow from ``restate_flow_warp_bwd``'s values: each half is the
    contraction gradient at q = fl(p + fl(flow noise)) (the product 1, the sum 1: the e_p of contract_bwd_bounds) of
    g = fl(dx3 + dx2) (1 when both consumers are present, else exact), times the noise (1)."""
    halves = []
    for h in st["halves"]:
        nz = np.abs(st["noise"])[:, None]
        e = contract_bwd_bounds(h) / UPDATE_SLACK
        halves.append(UPDATE_SLACK * (nz * e + np.where(e > 0, _r(h["out"] * st["noise"][:, None]), 0.0)))
    return np.concatenate(halves, 1)
