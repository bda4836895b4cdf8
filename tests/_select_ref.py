"""numpy / Python-integer models of the order-statistic entry points (csrc/select.hip, ``ops.order_statistics`` / ``quantile`` /
``weighted_percentile``), written from the rules in include/emernerf_hip.h and not from the kernel.

  * order statistics: ``np.sort`` (NaN last); zeros compare by value (the device returns +0 for either zero).
  * ``quantile``: torch's ``linear`` rule restated: rank = float32(q) * float32(n - 1) in fp32, a / b the order statistics at
    floor / ceil, w = rank - floor, d = b - a, ``fma(w, d, a)`` for w < 0.5 else ``fma(-d, 1 - w, b)``, NaN if the input holds one.
    The fma is an fp64 product (exact for fp32 factors) and an fp64 sum, rounded to fp32 once more.
  * weighted percentile: equal values merged into one node, weights quantised to integers of 2^-32 and summed as Python integers;
    t = p * (total / 100) in fp64; hi = the first node whose cumulative weight exceeds t (none: the largest value), lo = the node
    before it whatever its weight (none: hi); lo + (t - cum_lo) / (cum_hi - cum_lo) * (hi - lo) in fp64, one rounding per operation.
  * ``percentile_interval``: where the reference's own fp32 ``cumsum`` may put a percentile (see the function).
"""
from __future__ import annotations

import numpy as np

F = np.float32


def order_statistics(x, ranks):
    """Values of the 0-based ranks of the flattened fp32 array, NaN last."""
    s = np.sort(np.asarray(x, dtype=F).reshape(-1))
    return s[np.asarray(ranks, dtype=np.int64)]


def quantile_ranks(q, n):
    """(floor rank, ceil rank, fp32 weight) of torch.quantile's linear rule; the ranks are clamped to n - 1."""
    rank = F(q) * F(n - 1)
    assert rank.dtype == F
    lo, hi = np.floor(rank), np.ceil(rank)
    return min(int(lo), n - 1), min(int(hi), n - 1), F(rank - lo)


def lerp(a, b, w, fused=True):
    """torch's lerp of two fp32 values with an fp32 weight: fused (one rounding after the exact product; the device) or unfused
    (product and sum rounded on their own; the CPU's vectorised path may take either)."""
    a, b, w = F(a), F(b), F(w)
    with np.errstate(all="ignore"):
        d = F(b - a)
        if w < F(0.5):
            x, y, z = w, d, a
        else:
            x, y, z = F(-d), F(F(1) - w), b
        if fused:
            return F(np.float64(x) * np.float64(y) + np.float64(z))
        return F(F(x * y) + z)


def quantile(x, q, fused=True):
    """The model of ``ops.quantile(x, q)`` over the flattened fp32 array (scalar q)."""
    x = np.asarray(x, dtype=F).reshape(-1)
    if np.isnan(x).any():
        return F(np.nan)
    s = np.sort(x)
    lo, hi, w = quantile_ranks(q, s.size)
    return lerp(s[lo], s[hi], w, fused)


def quantise_weights(w):
    """Python integers rint(clamp(w, 0, 1) * 2^32), NaN as 0."""
    w = np.asarray(w, dtype=F).reshape(-1)
    w = np.where(np.isnan(w), F(0), np.clip(w, F(0), F(1))).astype(np.float64)
    return [int(v) for v in np.rint(w * 4294967296.0)]


def merged_nodes(x, w=None):
    """(ascending distinct values as fp32, Python-integer cumulative weights) -- -0 counts as +0, NaN last as one node."""
    x = np.asarray(x, dtype=F).reshape(-1)
    x = np.where(x == 0, F(0), x)
    q = [1] * x.size if w is None else quantise_weights(w)
    order = np.argsort(x, kind="stable")
    vals, cums, run = [], [], 0
    for i in order:
        v = x[i]
        same = bool(vals) and (vals[-1] == v or (np.isnan(vals[-1]) and np.isnan(v)))
        run += q[i]
        if same:
            cums[-1] = run
        else:
            vals.append(v)
            cums.append(run)
    return vals, cums


def percentile_from_nodes(vals, cums, p, t=None):
    """The weighted percentile p (or the value at the cumulative weight ``t``) of merged nodes, fp64."""
    total = cums[-1]
    if t is None:
        t = np.float64(p) * (np.float64(total) / np.float64(100.0))
    t = np.float64(t)
    k = next((i for i, c in enumerate(cums) if c > t), None)       # Python compares an integer and a float exactly
    if k is None:
        return np.float64(vals[-1])
    hi = np.float64(vals[k])
    if k == 0:
        return hi
    lo = np.float64(vals[k - 1])
    with np.errstate(all="ignore"):
        frac = (t - np.float64(cums[k - 1])) / np.float64(cums[k] - cums[k - 1])
        return lo + frac * (hi - lo)


def weighted_percentile(x, w, ps):
    vals, cums = merged_nodes(x, w)
    return np.array([percentile_from_nodes(vals, cums, p) for p in ps], dtype=np.float64)


def percentile_interval(x, w, p):
    """[M(t (1 - g)), M(t (1 + g))] for the model M and g = 2 n 2^-24 + 2^-20: where the reference's percentile may lie.  Its
    ``np.cumsum`` adds n non-negative fp32 terms one after another, so every prefix -- the total included -- carries a relative
    error of at most (n - 1) 2^-24; reading exact sums at t (1 -+ g) covers both errors (and the 2^-32 quantisation of the
    weights, which is far below 2^-20 of any prefix that matters) because M is monotonic in t."""
    vals, cums = merged_nodes(x, w)
    n = np.asarray(x).size
    g = 2 * n * 2.0 ** -24 + 2.0 ** -20
    t = np.float64(p) * (np.float64(cums[-1]) / 100.0)
    return percentile_from_nodes(vals, cums, None, t * (1 - g)), percentile_from_nodes(vals, cums, None, t * (1 + g))


def ulp(x):
    return np.spacing(np.abs(F(x)))


def quantile_bound(a, b):
    """2 ulp of max(|a|, |b|): the unfused lerp rounds a product bounded by 2 max and then a sum."""
    return 2.0 * float(ulp(max(abs(float(a)), abs(float(b)))))
