"""Exact-arithmetic probes and the bf16x3 emulation for the MLP head kernels (test helper, not a test module).

The heads run fp32 GEMMs on the bf16 matrix pipe: every fp32 operand is split into three bf16 planes, v = v_h + v_m + v_l,
and a product is the six partial products w_l x_h, w_h x_l, w_m x_m, w_m x_h, w_h x_m, w_h x_h accumulated in fp32
(csrc/mlp_fused.hip, "Arithmetic [r3]").  The rest runs on the fp32-input matrix cores or the VALU.

Exact probes.  If every operand lies on a fixed-point grid (A on 2^-qa, B on 2^-qb, bias on 2^-(qa+qb)), every split plane
lies on that grid too (a plane is an RNE rounding of a grid value to 8 significant bits, or a difference of two), so every
partial product is a multiple of the unit 2^-(qa+qb).  If moreover sum_k P(a) P(b) + |bias| < 2^24 units for an output
entry, with P(v) = |v_h| + |v_m| + |v_l| >= |v| the magnitude of v's planes, every partial sum of its partial products --
in ANY order, with any rounding inside a matrix instruction, or as fp32 fmaf products -- is an integer count of units
below 2^24, i.e. exactly representable in fp32.  A
correct kernel then returns bitwise the fp64 result cast to fp32, provided the three dropped products (w_m x_l, w_l x_m,
w_l x_l) are zero, which the probes arrange by giving one operand of each probe at most 17 significant bits (its l plane
is empty).  The builders below choose which plane pairs carry the value:

    "lh": A (weights) 20-bit, B rows with <= 6 entries +-1          -> w_l x_h, w_m x_h, w_h x_h
    "hl": A rows with <= 4 entries +-1, B 20-bit                      -> w_h x_l, w_h x_m, w_h x_h
    "mm": A 10-bit, B rows with <= 6 entries of 10 bits              -> w_m x_m, w_m x_h, w_h x_m, w_h x_h

Plane occupancy is checked on the inputs (``occupancy``), never assumed from the bit count.  tests/test_head_bounds_cpu.py
proves on the CPU that these inputs separate the six-product kernel from each of its plausible mutants.
"""
import numpy as np

U = 2.0 ** -24
BUDGET = 2.0 ** 24          # sum of plane magnitudes in grid units below which an entry must be exact
PRODUCTS = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))  # (A plane, B plane), smallest first
KINDS = ("lh", "hl", "mm")


# ------------------------------------------------------------------------------------------------------------ emulation
def bf16_rne(x) -> np.ndarray:
    """fp32 -> the fp32 value of its bf16 rounding (round to nearest even, v_cvt_pk_bf16_f32), through bit operations."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def split3(x):
    """x -> (h, m, l) fp32 arrays holding bf16 values, x = h + m + l (+ <= 2^-24 |x|); both subtractions are exact."""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = bf16_rne(r)
    s = (r - m).astype(np.float32)
    return h, m, bf16_rne(s)


def occupancy(x) -> dict:
    """Fraction of the NON-ZERO entries of x whose m / l plane is non-zero."""
    x = np.asarray(x, np.float32).reshape(-1)
    x = x[x != 0]
    if x.size == 0:
        return {"m": 0.0, "l": 0.0}
    _, m, l = split3(x)
    return {"m": float((m != 0).mean()), "l": float((l != 0).mean())}


def emu_gemm(a, b, bias=None, drop=(), zero_l=None, l_next=False, ks=32) -> np.ndarray:
    """out[m, n] = bias[n] + sum_k a[n, k] b[m, k] as the kernels evaluate it: the six partial products of the split planes
    (``PRODUCTS``), K in k-steps of ``ks``, every addition rounded to fp32 (products of two bf16 values are exact in fp32).

    Mutants: ``drop`` -- product pairs left out, e.g. {("l", "h")}; ``zero_l`` -- "a" / "b": that operand's l plane read as
    zero; ``l_next`` -- A's l plane read from the NEXT k-step (zero past the end)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    N, K = a.shape
    M = b.shape[0]
    pa, pb = dict(zip("hml", split3(a))), dict(zip("hml", split3(b)))
    if zero_l == "a":
        pa["l"] = np.zeros_like(pa["l"])
    if zero_l == "b":
        pb["l"] = np.zeros_like(pb["l"])
    if l_next:
        pa["l"] = np.concatenate([pa["l"][:, ks:], np.zeros((N, min(ks, K)), np.float32)], 1)[:, :K]
    acc = np.zeros((M, N), np.float32) if bias is None else np.broadcast_to(np.asarray(bias, np.float32), (M, N)).copy()
    for s in range(0, K, ks):
        for pw, px in PRODUCTS:
            if (pw, px) in drop:
                continue
            for k in range(s, min(s + ks, K)):
                acc = (acc + pb[px][:, k][:, None] * pa[pw][:, k][None, :]).astype(np.float32)
    return acc


def emu_fma_chain(a, b, bias=None) -> np.ndarray:
    """fp32-input MFMA: bitwise a k-ordered fmaf chain (emulated in fp64 then rounded per step: fma = one rounding)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((b.shape[0], a.shape[0]), np.float32) if bias is None else np.broadcast_to(np.asarray(bias, np.float32), (b.shape[0], a.shape[0])).copy()
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + b[:, k][:, None].astype(np.float64) * a[:, k][None, :]).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------------------ builders
def grid_values(rng, shape, bits: int, frac_bits: int, nonzero: bool = True) -> np.ndarray:
    """Integers in (-2^bits, 2^bits) (non-zero unless ``nonzero`` is False) times 2^-frac_bits, as fp32."""
    v = rng.integers(-(1 << bits) + 1, 1 << bits, size=shape)
    if nonzero:
        v[v == 0] = 1
    return (v * 2.0 ** -frac_bits).astype(np.float32)


def sparse_rows(rng, rows: int, cols: int, nnz: int, values, col_cap: int = 0) -> np.ndarray:
    """rows x cols with 0..nnz non-zeros per row (some rows empty) taken from ``values`` (same shape, or a scalar +-1);
    col_cap > 0: at most that many non-zeros per column too."""
    out = np.zeros((rows, cols), np.float32)
    vals = np.broadcast_to(np.asarray(values, np.float32), (rows, cols))
    used = np.zeros(cols, np.int64)
    for r in range(rows):
        k = int(rng.integers(0, nnz + 1)) if r % 7 else nnz   # every 7th row full, a few rows empty
        free = np.flatnonzero(used < col_cap) if col_cap > 0 else np.arange(cols)
        cs = rng.choice(free, size=min(k, free.size), replace=False)
        sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=cs.size)
        out[r, cs] = sign * np.abs(vals[r, cs])
        used[cs] += 1
    return out


def probe(kind: str, n_out: int, k: int, rows: int, seed: int, bias: bool = True):
    """(A [n_out, k] weights, B [rows, k] activations, bias [n_out] or None, qa, qb) for probe ``kind`` (module docstring)."""
    rng = np.random.default_rng(seed)
    if kind == "lh":
        a, qa = grid_values(rng, (n_out, k), 20, 20), 20
        b, qb = sparse_rows(rng, rows, k, 6, 1.0), 0
    elif kind == "hl":
        a, qa = sparse_rows(rng, n_out, k, max(1, min(4, 4 * k // n_out)), 1.0, col_cap=4), 0
        b, qb = grid_values(rng, (rows, k), 20, 20), 20
        b[rng.random(rows) < 0.05] = 0.0   # a few empty rows
    elif kind == "mm":
        a, qa = grid_values(rng, (n_out, k), 10, 10), 10
        b, qb = sparse_rows(rng, rows, k, 6, grid_values(rng, (rows, k), 10, 10)), 10
    else:
        raise ValueError(kind)
    c = grid_values(rng, (n_out,), 20, qa + qb, nonzero=False) if bias else None
    return a, b, c, qa, qb


def operand_like(kind: str, rows: int, cols: int, seed: int, role: str) -> np.ndarray:
    """The ``role`` ("a" or "b") operand distribution of probe ``kind``, rows x cols: the gradients that meet the weights in
    a backward GEMM take the B role of the same probe, so that the same plane pairs carry the value."""
    rng = np.random.default_rng(seed)
    if (kind, role) == ("lh", "b"):
        return sparse_rows(rng, rows, cols, 6, 1.0)
    if (kind, role) == ("hl", "a"):
        return sparse_rows(rng, rows, cols, max(1, min(4, 4 * cols // rows)), 1.0, col_cap=4)
    if kind in ("lh", "hl"):
        return grid_values(rng, (rows, cols), 20, 20)
    return sparse_rows(rng, rows, cols, 6, grid_values(rng, (rows, cols), 10, 10)) if role == "b" else grid_values(rng, (rows, cols), 10, 10)


def grid_q(kind: str, role: str) -> int:
    """Fraction bits of the ``role`` operand of probe ``kind``."""
    return {("lh", "a"): 20, ("lh", "b"): 0, ("hl", "a"): 0, ("hl", "b"): 20, ("mm", "a"): 10, ("mm", "b"): 10}[(kind, role)]


def signed_perm(n_out: int, n_in: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """n_out x n_in copy matrix: row j has one entry +-scale (scale a power of two) in column perm(j) (perm wraps when
    n_out > n_in, so every input is copied at least once when n_out >= n_in)."""
    rng = np.random.default_rng(seed)
    w = np.zeros((n_out, n_in), np.float32)
    reps = -(-n_out // n_in)
    cols = np.concatenate([rng.permutation(n_in) for _ in range(reps)])[:n_out]
    w[np.arange(n_out), cols] = rng.choice(np.array([-scale, scale], np.float32), size=n_out)
    return w


def positive_copy(n_out: int, n_in: int) -> np.ndarray:
    """n_out x n_in: unit j < n_in copies +x_j, unit n_in <= j < 2 n_in copies -x_(j - n_in), the rest are zero: after a
    ReLU every non-zero input lives in exactly one unit (with its magnitude), so sparsity and bit counts carry over."""
    w = np.zeros((n_out, n_in), np.float32)
    j = np.arange(min(n_out, 2 * n_in))
    w[j, j % n_in] = np.where(j < n_in, 1.0, -1.0)
    return w


def grid_of(x) -> int:
    """The smallest q such that every entry of x is a multiple of 2^-q (0 for an all-zero x)."""
    x = np.asarray(x, np.float64).reshape(-1)
    x = x[x != 0]
    if x.size == 0:
        return 0
    m, e = np.frexp(np.abs(x))
    i = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((i & -i).astype(np.float64)).astype(np.int64)
    return int((53 - e - tz).max())


def units(a, b, bias=None) -> np.ndarray:
    """abs_units of the GEMM b a^T (+ bias) on the finest grid its operands lie on (bias must lie on it too)."""
    q = grid_of(a) + grid_of(b)
    if bias is not None:
        assert grid_of(bias) <= q, "bias off the product grid"
    return abs_units(a, b, bias, q)


# ------------------------------------------------------------------------------------------------------------ checking
def on_grid(x, q: int) -> bool:
    """Every entry of x is a multiple of 2^-q."""
    v = np.asarray(x, np.float64) * 2.0 ** q
    return bool(np.all(v == np.round(v)))


def plane_mag(x) -> np.ndarray:
    """|x_h| + |x_m| + |x_l| in fp64 (>= |x|; equal unless the signed-digit split overshoots)."""
    return sum(np.abs(p.astype(np.float64)) for p in split3(x))


def abs_units(a, b, bias, q: int) -> np.ndarray:
    """sum_k P(a[n, k]) P(b[m, k]) + |bias[n]| in units of 2^-q, [rows, n_out] (fp64: exact far beyond the budget)."""
    s = plane_mag(b) @ plane_mag(a).T
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    return s * 2.0 ** q


def assert_exact(name: str, got, ref, units=None, min_cover: float = 1.0, report: dict = None) -> float:
    """Entries with ``units`` < BUDGET (all entries when units is None) must equal fp32(ref) bit for bit, and ref must be
    exactly representable in fp32 there; at least ``min_cover`` of the entries must be in budget.  Returns the cover."""
    got = np.asarray(got, np.float32).reshape(-1) + np.float32(0.0)   # + 0: -0.0 -> +0.0 (the sign of an exact zero is not compared)
    ref = np.asarray(ref, np.float64).reshape(-1) + 0.0
    sel = np.ones(ref.shape, bool) if units is None else (np.asarray(units, np.float64).reshape(-1) < BUDGET)
    cover = float(sel.mean()) if sel.size else 1.0
    assert cover >= min_cover, f"{name}: only {cover:.3f} of the entries are inside the exact budget (< {min_cover})"
    r32 = ref.astype(np.float32)
    assert np.array_equal(r32[sel].astype(np.float64), ref[sel]), f"{name}: reference not representable in fp32 (probe broken)"
    bad = sel & (got.view(np.uint32) != r32.view(np.uint32))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {int(sel.sum())} exact entries differ from the exact result; first at "
                             f"flat index {i}: got {got[i]!r}, exact {r32[i]!r}, diff {float(got[i]) - ref[i]:.3e}")
    if report is not None:
        report[name] = cover
    return cover


def assert_ulp(name: str, got, want, k: float):
    """|got - want| <= k u |want| per entry (want in fp64; infinities must match exactly)."""
    got = np.asarray(got, np.float64).reshape(-1)
    want = np.asarray(want, np.float64).reshape(-1)
    inf = ~np.isfinite(want)
    assert np.array_equal(got[inf], want[inf]), f"{name}: non-finite entries differ"
    g, w = got[~inf], want[~inf]
    err = np.abs(g - w)
    lim = k * U * np.abs(w)
    bad = ~(err <= lim)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} entries beyond {k} u relative; first: got {g[i]!r}, want {w[i]!r}, "
                             f"err {err[i] / max(U * abs(w[i]), 1e-300):.2f} u")


# ------------------------------------------------------------------------------------- fp64 reference of a Linear stack
def mlp_ref(x, Ws, Bs, relus):
    """Forward of Linear (+ ReLU where relus[i]) in fp64; asserts every layer's pre-activations inside the exact budget (a
    probe whose forward is not exact is broken, not a finding).  Returns (inputs of each layer, pre-activations)."""
    hs, pres = [np.asarray(x, np.float64)], []
    for i, (w, b) in enumerate(zip(Ws, Bs)):
        w = np.asarray(w, np.float64)
        pre = hs[-1] @ w.T + (0.0 if b is None else np.asarray(b, np.float64))
        u = units(w, hs[-1], b)
        assert (u < BUDGET).all(), f"probe broken: layer {i} forward leaves the exact budget ({u.max() / BUDGET:.2f} x)"
        pres.append(pre)
        hs.append(np.maximum(pre, 0.0) if relus[i] else pre)
    return hs, pres


def mlp_ref_bwd(hs, pres, Ws, relus, g, row_ok=None):
    """fp64 backward of ``mlp_ref`` for the output gradient g; relu'(0) = 0 as in torch.  Returns {name: (value, ok)} for
    dW<i>, db<i> and dx, where ``ok`` marks the entries a correct kernel must return EXACTLY: the entry's own GEMM is inside
    the budget and every gradient entry feeding it was exact itself.  row_ok: rows of g that are not exact (e.g. a side
    gradient through an inexact exp)."""
    n = len(Ws)
    d = np.asarray(g, np.float64)
    ok = np.ones(d.shape, bool) if row_ok is None else np.broadcast_to(np.asarray(row_ok, bool)[:, None], d.shape).copy()
    out = {}
    for i in reversed(range(n)):
        if relus[i]:
            live = pres[i] > 0
            d = d * live
            ok = ok | ~live
        w = np.asarray(Ws[i], np.float64)
        bad = np.where(ok, 0.0, np.abs(d))                   # contributions of inexact gradient entries
        uw = units(d.T, hs[i].T).T
        out[f"dW{i}"] = (d.T @ hs[i], (uw < BUDGET) & ((bad.T @ np.abs(hs[i])) == 0))
        ub = plane_mag(d).sum(0) * 2.0 ** grid_of(d)
        out[f"db{i}"] = (d.sum(0), (ub < BUDGET) & (bad.sum(0) == 0))
        ud = units(w.T, d)
        ok = (ud < BUDGET) & ((bad @ np.abs(w)) == 0)
        d = d @ w
    out["dx"] = (d, ok)
    return out
