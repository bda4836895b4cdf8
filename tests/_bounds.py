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
