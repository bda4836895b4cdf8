"""Exact-arithmetic probes, a numpy model and the references of the proposal-loss kernel (test helper, not a test module).

``emer_prop_loss`` (emernerf_amd/csrc/proploss.hip) gives one wavefront per ray: the sorted halves s - r and s + r are
merged by binary-search ranks, three 64-wide chunked wave scans with register carries give the slope, the blurred pdf and
the blurred cdf at the 2 (n + 1) knots, every proposal edge is bracketed by a further binary search and interpolated
quadratically, then the hinge, its gradient G = d term / d w_p and d cdf_j = (G_{j-1} - G_j) scale.  Mode 1 is the plain
histogram loss with LDS atomics.

Exact probes.  With dyadic inputs (``build``) every intermediate up to and including the hinge argument
d = max(w_s - w_p, 0) is exactly representable in fp32, and every partial sum of the three scans -- in ANY order -- is an
integer count of units below 2^24.  A correct kernel then holds d bitwise, only correctly rounded operations follow, and
the results are held to a few units of 2^-24 (tests/_bounds.py c_prop_*).  ``check_ray`` asserts these preconditions on the
inputs themselves (fp64 evaluation, every named intermediate equal to its fp32 cast, scan abs-sums in units).

``model`` is the kernel's algorithm in numpy, in the kernel's operation order, in fp32 (the emulation) or fp64 (the stage
values the bounds are built from); ``MUTANTS`` lists its plausible slips.  ``ref_aa`` / ``ref_pdf`` are the references:
oracle/ref_path.prop_loss (torch.sort, masked max / min, autograd) and the torch restatement of _pdf_loss, in float64 or
float32 on copies of the same fp32 inputs.  tests/test_prop_loss_bounds_cpu.py shows without a GPU that the probes
separate the correct model from every mutant.
"""
import math

import numpy as np
import torch

from tests._head_probe import grid_of

F32 = np.float32
F64 = np.float64
BUDGET = 2.0 ** 24
EPS_AA, EPS_PDF = 1e-5, 1e-7

# name -> what it changes in ``model`` (mode 0 unless noted)
MUTANTS = {
    "tie": "both merge ranks by lower_bound: tied knots collide, one is lost",
    "carry_slope": "slope scan: carry dropped at the 64-lane chunk boundary",
    "carry_pdf": "pdf scan: carry dropped at the chunk boundary",
    "carry_cdf": "cdf scan: carry dropped at the chunk boundary",
    "w_first": "w_{-1} = w_0 instead of 0 in the slope events",
    "w_last": "w_n = w_{n-1} instead of 0 in the slope events",
    "shift": "gradient written one edge late",
    "G2": "second term of G (d^2 / den^2) dropped",
    "eps": "the epsilons of the two modes swapped (1e-7 for 1e-5)",
}
# Mutants that CANNOT fail on exact inputs (asserted bitwise equal in the CPU test), with the reason:
EQUIVALENT = {
    "bracket_lower": "step 4 bracketing by lower_bound: an edge on a knot is then interpolated from the segment to its left, "
                     "and the piecewise quadratic is continuous at the knots (exact on the probes: same value)",
    "noclip": "the clip of off: with the den == 0 branch taken apart, x0 <= q < x1 gives 0 <= num / den < 1 already",
    "den0": "den == 0 returning 0 for a positive numerator: den == 0 only happens right of the last (left of the first) knot, "
            "where i0 == i1, p0 == p1 and p0 + p1 off + p0 (1 - off) = 2 p0 for every off",
}
MUTANTS_PDF = {
    "eps": "the epsilons of the two modes swapped (1e-5 for 1e-7)",
    "left": "searchsorted(right=False): a final edge equal to a proposal edge lands one bracket lower",
    "noclamp": "ids_left not clamped at 0",
}


# ---------------------------------------------------------------------------------------------------------- the model
def _scan(v, dt, drop_carry=False):
    """Inclusive scan as the kernel does it: 64-lane Hillis-Steele steps (offsets 1, 2, ... 32), chunk after chunk, the
    running total carried in a register (lane 63 of the previous chunk)."""
    n = v.size
    out = np.empty(n, dt)
    carry = dt(0)
    for base in range(0, n, 64):
        k = min(64, n - base)
        w = np.zeros(64, dt)
        w[:k] = v[base:base + k]
        off = 1
        while off < 64:
            o = w.copy()
            w[off:] = (w[off:] + o[:-off]).astype(dt)
            off <<= 1
        w = (w + (dt(0) if drop_carry else carry)).astype(dt)
        out[base:base + k] = w[:k]
        carry = w[63]
    return out


def _wave_sum(terms, dt):
    """Per-lane sequential sums over j = lane, lane + 64, ... then the xor butterfly (32, 16, ... 1); lane 0."""
    part = np.zeros(64, dt)
    for base in range(0, terms.size, 64):
        k = min(64, terms.size - base)
        part[:k] = (part[:k] + terms[base:base + k]).astype(dt)
    lanes = np.arange(64)
    off = 32
    while off:
        part = (part + part[lanes ^ off]).astype(dt)
        off >>= 1
    return part[0]


def model(s, trans, q, pc, pulse, scale, dt=F32, mut=""):
    """Mode 0 of prop_loss_kernel for ONE ray, every operation in ``dt``.  Returns a dict of the stages (knots ``xr``,
    events ``ev``, ``slope``, ``dx``, ``pdf``, ``area``, ``cdf``, ``ci``, ``ws``, ``wp``, ``d``, ``G``, ``term``, ``loss``,
    ``grad``, and the sub-expressions the exactness check looks at)."""
    s, trans, q, pc = (np.asarray(a, dt) for a in (s, trans, q, pc))
    n, m = trans.size, q.size - 1
    ne, K = n + 1, 2 * (n + 1)
    r, one = dt(pulse), dt(1)
    st = {}
    c = np.concatenate([one - trans, [one]]).astype(dt)
    A, B = (s - r).astype(dt), (s + r).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        wn = ((c[1:] - c[:-1]) / (s[1:] - s[:-1])).astype(dt)
    wr, wl = np.append(wn, dt(0)), np.insert(wn, 0, dt(0))
    if mut == "w_first":
        wl[0] = wn[0]
    if mut == "w_last":
        wr[n] = wn[n - 1]
    y = ((wr - wl) / (dt(2) * r)).astype(dt)
    j = np.arange(ne)
    pa = j + np.searchsorted(B, A, "left")
    pb = j + np.searchsorted(A, B, "left" if mut == "tie" else "right")
    xr, ev = np.zeros(K, dt), np.zeros(K, dt)
    xr[:ne], ev[:ne] = s, c          # (the kernel borrows these rows as scratch first: what a lost slot would still hold)
    xr[pa], ev[pa] = A, y
    xr[pb], ev[pb] = B, -y
    slope = _scan(ev[:K - 1], dt, mut == "carry_slope")
    dx = (xr[1:] - xr[:-1]).astype(dt)
    v = (dx * slope).astype(dt)
    pdf = np.concatenate([[dt(0)], np.maximum(_scan(v, dt, mut == "carry_pdf"), dt(0))]).astype(dt)
    psum = (pdf[1:] + pdf[:-1]).astype(dt)
    area = ((dt(0.5) * psum).astype(dt) * dx).astype(dt)
    cdf = np.concatenate([[dt(0)], _scan(area, dt, mut == "carry_cdf")]).astype(dt)
    k = np.searchsorted(xr, q, "left" if mut == "bracket_lower" else "right")
    i0, i1 = np.maximum(k - 1, 0), np.minimum(k, K - 1)
    x0, x1, p0, p1 = xr[i0], xr[i1], pdf[i0], pdf[i1]
    num, den = (q - x0).astype(dt), (x1 - x0).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        quo = (num / den).astype(dt)
    fin = quo if mut == "noclip" else np.clip(quo, dt(0), one)
    at0 = np.zeros_like(num) if mut == "den0" else np.where(num > 0, one, dt(0))
    off = np.where(den == 0, at0, fin).astype(dt)
    t1 = (p1 * off).astype(dt)
    om = (one - off).astype(dt)
    t2 = (p0 * om).astype(dt)
    inner = ((p0 + t1).astype(dt) + t2).astype(dt)
    prod = (num * inner).astype(dt)
    ci = (cdf[i0] + (prod / dt(2)).astype(dt)).astype(dt)
    ws, wp = (ci[1:] - ci[:-1]).astype(dt), (pc[1:] - pc[:-1]).astype(dt)
    d = np.maximum((ws - wp).astype(dt), dt(0))
    dn = (wp + dt(F32(EPS_PDF if mut == "eps" else EPS_AA))).astype(dt)
    term = ((d * d).astype(dt) / dn).astype(dt)
    G = ((dt(-2) * d).astype(dt) / dn).astype(dt)
    if mut != "G2":
        G = (G - ((d * d).astype(dt) / (dn * dn).astype(dt)).astype(dt)).astype(dt)
    loss = dt(_wave_sum(term, dt) * dt(scale))
    grad = ((np.insert(G, 0, dt(0)) - np.append(G, dt(0))).astype(dt) * dt(scale)).astype(dt)
    if mut == "shift":
        grad = np.insert(grad[:-1], 0, dt(0))
    st.update(s=s, pulse=float(pulse), pa=pa, pb=pb, c=c, A=A, B=B, wn=wn, y=y, xr=xr, ev=ev, slope=slope, dx=dx, v=v, pdf=pdf, psum=psum, area=area, cdf=cdf, i0=i0, i1=i1,
              num=num, den=den, off=off, t1=t1, om=om, t2=t2, inner=inner, prod=prod, ci=ci, ws=ws, wp=wp, d=d, dn=dn, term=term, G=G,
              loss=loss, grad=grad)
    return st


def model_pdf(s, trans, q, pc, scale, dt=F32, mut=""):
    """Mode 1 (_pdf_loss) for ONE ray.  ``hits`` / ``gabs``: per proposal entry, the number of atomics and the sum of their
    magnitudes (the LDS atomics land in any order)."""
    s, trans, q, pc = (np.asarray(a, dt) for a in (s, trans, q, pc))
    n, m = trans.size, q.size - 1
    c = np.concatenate([dt(1) - trans, [dt(1)]]).astype(dt)
    ub = np.searchsorted(q, s, "left" if mut == "left" else "right")
    il = ub[:-1] - 1
    il = np.minimum(il, m) if mut == "noclamp" else np.clip(il, 0, m)      # (index -1 wraps to the last entry)
    ir = np.minimum(ub[1:], m)
    w, wo = (c[1:] - c[:-1]).astype(dt), (pc[ir] - pc[il]).astype(dt)
    d = np.maximum((w - wo).astype(dt), dt(0))
    dn = (w + dt(F32(EPS_AA if mut == "eps" else EPS_PDF))).astype(dt)
    term = ((d * d).astype(dt) / dn).astype(dt)
    g = ((dt(-2) * d).astype(dt) / dn).astype(dt)
    G, hits, gabs = np.zeros(m + 1, dt), np.zeros(m + 1, np.int64), np.zeros(m + 1, F64)
    for jj in np.flatnonzero(g != 0):
        G[ir[jj]] = dt(G[ir[jj]] + g[jj])
        G[il[jj]] = dt(G[il[jj]] - g[jj])
        for e in (ir[jj], il[jj]):
            hits[e] += 1
            gabs[e] += abs(float(g[jj]))
    return dict(c=c, il=il, ir=ir, w=w, wo=wo, d=d, dn=dn, term=term, g=g, G=G, hits=hits, gabs=gabs,
                loss=dt(_wave_sum(term, dt) * dt(scale)), grad=(G * dt(scale)).astype(dt))


# ------------------------------------------------------------------------------------------------------- references
def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, F32))).to(dtype)


def ref_aa(s_fin, trans, s_p, c_p, pulse, scale, dtype=torch.float64):
    """oracle.ref_path.prop_loss on ``dtype`` copies of the fp32 inputs, one ray at a time: (loss_rays [R], grad [R, m+1])
    with loss_rays[r] = scale sum_j term_rj, as float64 numpy."""
    from oracle.ref_path import prop_loss
    sf, tr, sp = _t(s_fin, dtype), _t(trans, dtype), _t(s_p, dtype)
    cp = _t(c_p, dtype).requires_grad_(True)
    m = cp.shape[1] - 1
    rays = []
    for r in range(sf.shape[0]):
        cache = [(sp[r:r + 1], cp[r:r + 1], 0), (sf[r:r + 1], None, None)]
        rays.append(prop_loss(cache, tr[r:r + 1], scale * m, pulse=(pulse,)))
    rays = torch.stack(rays)
    rays.sum().backward()
    return rays.detach().double().numpy(), cp.grad.double().numpy()


def ref_stages(s_fin, trans, s_p, pulse, dtype=torch.float64):
    """The reference's own blurred pdf / cdf at its knots and the interpolated cdf at the proposal edges (ref_path
    blur_stepfun / sorted_interp_quad), as float64 numpy: (knots, pdf, cdf, ci)."""
    from oracle.ref_path import blur_stepfun, sorted_interp_quad
    sf, tr, sp = _t(s_fin, dtype), _t(trans, dtype), _t(s_p, dtype)
    cd = 1.0 - torch.cat([tr, torch.zeros_like(tr[..., :1])], -1)
    wn = (cd[..., 1:] - cd[..., :-1]) / (sf[..., 1:] - sf[..., :-1])
    x, w = blur_stepfun(sf, wn, pulse)
    area = 0.5 * (w[..., 1:] + w[..., :-1]) * (x[..., 1:] - x[..., :-1])
    c = torch.cat([torch.zeros_like(area[..., :1]), torch.cumsum(area, -1)], -1)
    ci = sorted_interp_quad(sp, x, w, c)
    return tuple(a.double().numpy() for a in (x, w, c, ci))


def ref_pdf(s_fin, trans, s_p, c_p, scale, dtype=torch.float64):
    """_pdf_loss restated in torch (searchsorted(right=True), both index sets clamped to [0, m]) on ``dtype`` copies:
    (loss_rays [R], grad [R, m+1]) as float64 numpy."""
    sf, tr, sp = _t(s_fin, dtype), _t(trans, dtype), _t(s_p, dtype)
    cp = _t(c_p, dtype).requires_grad_(True)
    m = cp.shape[1] - 1
    cq = 1.0 - torch.cat([tr, torch.zeros_like(tr[..., :1])], -1)
    ir = torch.searchsorted(sp.contiguous(), sf.contiguous(), right=True)
    il = (ir - 1).clamp(0, m)
    ir = ir.clamp(0, m)
    w = cq[:, 1:] - cq[:, :-1]
    wo = cp.gather(-1, ir[:, 1:]) - cp.gather(-1, il[:, :-1])
    rays = (torch.clip(w - wo, min=0) ** 2 / (w + EPS_PDF)).sum(-1) * scale
    rays.sum().backward()
    return rays.detach().double().numpy(), cp.grad.double().numpy()


# ----------------------------------------------------------------------------------------------------------- builders
FAMILIES = ("tie", "alt", "block", "zeros", "spike", "short", "onknot", "zerowidth", "zero_wp")
SHAPES = ((1, 1), (2, 1), (31, 63), (32, 64), (48, 40), (64, 65), (100, 64), (128, 128))
RAYS = (1, 4, 13)


def family_pulse(family, n, seed):
    """The (power of two) pulse half-width of a probe batch: 2^-5 / 2^-8 (the dyadic neighbours of the shipped 0.03 /
    0.003) unless the family is about the merge pattern."""
    if family == "alt":      # 2 r below the smallest spacing: A and B alternate strictly
        return 2.0 ** -(_grid_bits(n, family) + 2)
    if family == "tie" and seed % 2:   # 2 r = the lattice spacing: s_i + r == s_{i+1} - r for every i
        return 2.0 ** -(_grid_bits(n, family) + 1)
    if family == "block":    # every s - r before every s + r (one tie, s_n - r == s_0 + r, on full support)
        return 0.5
    return 2.0 ** -5 if seed % 2 == 0 else 2.0 ** -8


def _grid_bits(n, family):
    if family == "tie":
        return max(5, math.ceil(math.log2(n))) if n > 1 else 5
    g = 7
    need = (n + 1) + (n + 1) // 4
    while (1 << g) // (2 if family == "short" else 1) < need:
        g += 1
    return g


def _final_samples(rng, n, family):
    """Final edges (distinct multiples of 2^-g), the normalised weights and the cdf, in fp64.  Interval ``f`` has a power
    of two width and receives 1 - cdf; the intervals behind it are saturated (weight 0, trans 0)."""
    g = _grid_bits(n, family)
    if family == "tie":                      # uniform lattice from 0
        ds_u = np.ones(n, np.int64)
        lo, f = 0, n - 1
    else:
        T = (1 << g) // (2 if family == "short" else 1)
        lo = (1 << g) // 4 if family == "short" else 0
        if n == 1:
            ds_u, f = np.array([T], np.int64), 0
        else:
            f = n - 1
            if family == "zeros" and n >= 6:
                f = n - 1 - max(1, n // 6)
            if family == "spike":
                f = int(rng.integers(0, n))
            p = int(min(math.floor(math.log2(T - (n - 1))), rng.integers(0, 4)))
            rem = T - (1 << p)
            cuts = np.sort(rng.choice(rem - 1, size=n - 2, replace=False)) + 1 if n > 2 else np.zeros(0, np.int64)
            other = np.diff(np.concatenate([[0], cuts, [rem]])).astype(np.int64)
            ds_u = np.insert(other, f, 1 << p)
    s = (lo + np.concatenate([[0], np.cumsum(ds_u)])) * 2.0 ** -g
    ds = ds_u * 2.0 ** -g
    a = np.where(rng.random(n) < 0.85, rng.integers(1, 7, n), 0)
    if family == "spike":
        a[:] = 0
    if family == "zeros" and n >= 6:
        run = max(1, n // 6)
        a[:run] = 0
        a[n // 2 - run // 2: n // 2 - run // 2 + run] = 0
    a[f:] = 0
    base = int((ds_u[:f] * a[:f]).sum())                       # units of 2^-(g + 2 + k)
    k = (math.ceil(math.log2(base + 1)) if base else 0) - (g + 2) + int(rng.integers(0, 2))
    w = a * 0.25 * 2.0 ** -k
    cdf = np.concatenate([[0.0], np.cumsum(ds * w)])
    cdf[f + 1:] = 1.0
    assert (np.diff(cdf) >= 0).all() and cdf[f] < 1.0 or base == 0
    return s, cdf, f


def build_ray(n, m, family, seed, pulse):
    """One probe ray: dict(s_fin [n+1], trans [n], s_p [m+1], c_p [m+1]) as fp32 (built in fp64, asserted representable)."""
    rng = np.random.default_rng(seed)
    s, cdf, f = _final_samples(rng, n, family)
    trans = 1.0 - cdf[:-1]
    for name, a in (("s_fin", s), ("trans", trans)):
        assert np.array_equal(a.astype(F32).astype(F64), a), f"probe broken: {name} not representable in fp32"
    assert np.array_equal(1.0 - trans, cdf[:-1])
    base = model(s, trans, [0.0, 1.0], [0.0, 0.0], pulse, 1.0, F64)
    x = base["xr"]
    knots = np.unique(x)
    if family == "onknot":
        cand = knots
    else:
        fr = np.array([0.0, 0.25, 0.5, 0.75])
        cand = np.unique(np.concatenate([(x[:-1, None] + (x[1:] - x[:-1])[:, None] * fr[None, :]).reshape(-1), x[-1:]]))
    if family == "short":       # 0 and 1 lie outside the knots: the den == 0 branches of step 4
        assert x[0] > 0.0 and x[-1] < 1.0
        inner = rng.choice(cand, size=m - 1, replace=cand.size < m - 1) if m > 1 else np.zeros(0)
        q = np.concatenate([[0.0], np.sort(inner), [1.0]])
    else:
        cand = cand[(cand >= 0.0) & (cand <= 1.0)] if pulse < 0.5 else cand
        q = np.sort(rng.choice(cand, size=m + 1, replace=cand.size < m + 1))
    dup = np.zeros(m, bool)
    if family == "zerowidth":
        for jj in rng.choice(m, size=max(1, m // 8), replace=False):
            q[jj + 1] = q[jj]
        q = np.sort(q)
        dup = np.diff(q) == 0
    ws = np.diff(model(s, trans, q, np.zeros(m + 1), pulse, 1.0, F64)["ci"])
    wp_u = np.maximum(np.floor(ws * 1024.0 + rng.uniform(-1.2, 1.8, m)), 0.0)
    if family == "zero_wp":
        wp_u[rng.random(m) < 0.3] = 0.0
    if family == "zerowidth":   # repeated edge with equal cdf, and with unequal cdf
        wp_u[dup] = np.arange(int(dup.sum())) % 2
    c_p = np.minimum(np.concatenate([[0.0], np.cumsum(wp_u)]), 1024.0) / 1024.0
    return dict(s_fin=s.astype(F32), trans=trans.astype(F32), s_p=q.astype(F32), c_p=c_p.astype(F32), pulse=pulse, family=family)


def _exact32(a):
    a = np.asarray(a, F64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(F32).astype(F64), a))


def check_ray(ray):
    """Assert the probe's preconditions and return its statistics: every value is on its grid (each named intermediate of
    the fp64 evaluation, up to the hinge argument, equals its fp32 cast), and for each of the three scans abs-sum / unit is
    below 2^24, so every partial sum in any order is exact."""
    st = model(ray["s_fin"], ray["trans"], ray["s_p"], ray["c_p"], ray["pulse"], 1.0, F64)
    for name in ("c", "A", "B", "wn", "y", "xr", "ev", "slope", "dx", "v", "pdf", "psum", "area", "cdf", "num", "den", "off", "t1",
                 "om", "t2", "inner", "prod", "ci", "ws", "wp", "d"):
        assert _exact32(st[name]), f"probe broken ({ray['family']}): {name} is not representable in fp32"
    K = st["xr"].size
    assert (np.diff(st["xr"]) >= 0).all(), "probe broken: knots not sorted"
    assert (st["pdf"] >= 0).all() and st["pdf"][-1] == 0.0, "probe broken: the clamp would act / the pdf does not return to 0"
    units = {}
    for name, terms in (("slope", st["ev"][:K - 1]), ("pdf", st["v"]), ("cdf", st["area"])):
        u = float(np.abs(terms).sum() * 2.0 ** grid_of(terms))
        assert u < BUDGET, f"probe broken ({ray['family']}): scan {name} has abs-sum / unit 2^{math.log2(u):.1f}"
        units[name] = u
    A, B = st["A"], st["B"]
    q, x = np.asarray(ray["s_p"], F64), st["xr"]
    return dict(units=units, ties=int(np.isin(A, B).sum()), active=float((st["d"] > 0).mean()), on_knot=int(np.isin(q, x).sum()),
                outside=int(((q < x[0]) | (q > x[-1])).sum()), zero_w=int((st["wn"] == 0).sum()), zero_wp=int((st["wp"] == 0).sum()),
                zero_width=int((np.diff(q) == 0).sum()), K=K)


def build(R, n, m, family, seed=0):
    """A batch of R probe rays of one family (one pulse per batch, as the kernel takes it): dict of [R, ...] fp32 arrays."""
    pulse = family_pulse(family, n, seed)
    rays = [build_ray(n, m, family, 1000 * seed + 17 * r + n + m, pulse) for r in range(R)]
    out = {k: np.stack([ray[k] for ray in rays]) for k in ("s_fin", "trans", "s_p", "c_p")}
    out.update(pulse=pulse, family=family, rays=rays)
    return out


# ---- pdf mode
def build_pdf_ray(n, m, kind, seed):
    """Mode 1 probe ray.  kind "shared": every proposal edge is also a final edge (decides searchsorted(right=True));
    "scatter": the proposal edges crowd into a corner, so that many final intervals land in the same two entries;
    "mixed": random dyadic edges."""
    rng = np.random.default_rng(seed)
    s, cdf, _ = _final_samples(rng, n, "plain")
    g = _grid_bits(n, "plain")
    if kind == "shared":
        q = np.sort(rng.choice(s, size=m + 1, replace=s.size < m + 1))
    elif kind == "scatter":
        q = np.sort(np.concatenate([[0.0], rng.integers(1, 1 << (g + 2), m - 1) * 2.0 ** -(g + 2) / 16.0, [1.0]]))[:m + 1] if m > 1 else np.array([0.0, 1.0])
    else:
        q = np.sort(rng.integers(0, (1 << (g + 1)) + 1, m + 1) * 2.0 ** -(g + 1))
    wp_u = rng.integers(0, max(2, 2048 // m), m)
    if kind == "scatter":
        wp_u[-1] = 1          # the wide last bracket carries little proposal mass: the final intervals inside it are active
    c_p = np.minimum(np.concatenate([[0.0], np.cumsum(wp_u)]), 1024.0) / 1024.0
    trans = 1.0 - cdf[:-1]
    assert _exact32(s) and _exact32(trans) and _exact32(q) and np.array_equal(1.0 - trans, cdf[:-1])
    return dict(s_fin=s.astype(F32), trans=trans.astype(F32), s_p=q.astype(F32), c_p=c_p.astype(F32), kind=kind)


def check_pdf_ray(ray):
    st = model_pdf(ray["s_fin"], ray["trans"], ray["s_p"], ray["c_p"], 1.0, F64)
    for name in ("c", "w", "wo", "d"):
        assert _exact32(st[name]), f"probe broken (pdf {ray['kind']}): {name} is not representable in fp32"
    s, q = np.asarray(ray["s_fin"], F64), np.asarray(ray["s_p"], F64)
    return dict(shared=int(np.isin(s[1:-1], q).sum()), max_hits=int(st["hits"].max()), active=float((st["d"] > 0).mean()))


def build_pdf(R, n, m, kind, seed=0):
    rays = [build_pdf_ray(n, m, kind, 1000 * seed + 31 * r + n + m) for r in range(R)]
    out = {k: np.stack([ray[k] for ray in rays]) for k in ("s_fin", "trans", "s_p", "c_p")}
    out.update(kind=kind, rays=rays)
    return out


# ------------------------------------------------------------------------------------------- realistic training inputs
def realistic(R, n, m, seed, oracle):
    """Rays shaped like a training step (section 3): a proposal histogram over m uniform intervals from a density with
    empty space in front, one or two thin walls and saturation behind the last wall (trans underflows to exactly 0), and
    final edges drawn from the proposal cdf by ``oracle.importance_sample`` (the CPU sampler: every test sees the same
    arrays).  Rays with a repeated final edge (0 / 0 in the reference) are rejected.  -> dict of [R, ...] fp32 arrays."""
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("s_fin", "trans", "s_p", "c_p")}
    tries = 0
    while len(out["s_fin"]) < R:
        tries += 1
        assert tries < 20 * R + 20, "realistic: too many rejected rays"
        sp = np.linspace(0.0, 1.0, m + 1).astype(F32)
        mid = 0.5 * (sp[1:] + sp[:-1]).astype(F64)
        dens = np.where(mid > 0.05, 0.3, 0.0)                     # haze the (blurrier) proposal believes in; nothing right at the camera
        walls = np.sort(rng.uniform(0.25, 0.7, size=int(rng.integers(1, 3))))
        sig = rng.uniform(0.004, 0.02, size=walls.size)
        for i, (w, sg) in enumerate(zip(walls, sig)):             # a last, opaque wall; before it perhaps a translucent one
            tau_w = rng.uniform(5.0, 9.0) if i == walls.size - 1 else rng.uniform(0.5, 2.0)
            dens += tau_w / (sg * math.sqrt(2.0 * math.pi)) * np.exp(-0.5 * ((mid - w) / sg) ** 2)
        dens[mid > walls[-1] + 3.0 * sig[-1]] = 60.0              # behind it the proposal cdf creeps up to exactly 1
        tau = np.concatenate([[0.0], np.cumsum(dens * np.diff(sp.astype(F64)))])
        c_p = (1.0 - np.exp(-tau)).astype(F32)
        c_p[-1] = 1.0
        jit = rng.random(1).astype(F32)
        s = oracle.importance_sample(sp[None, :], c_p[None, :], n, jit)[0]
        if not (np.diff(s) > 0).all():
            continue
        # the final level sees a sharper version of the same scene
        sm = 0.5 * (s[1:] + s[:-1]).astype(F64)
        fd = np.interp(sm, mid, dens) * rng.uniform(0.7, 1.4)
        fd[sm < walls[0] - 3.0 * sig[0]] = 0.0                     # ... is empty in front of the first wall (trans == 1 exactly)
        fd[sm > walls[-1]] = 3e5                                   # ... and saturates behind the last one (trans underflows to 0)
        ft = np.concatenate([[0.0], np.cumsum(fd * np.diff(s.astype(F64)))])[:-1]
        trans = np.exp(-ft).astype(F32)
        for k, a in zip(("s_fin", "trans", "s_p", "c_p"), (s, trans, sp, c_p)):
            out[k].append(np.asarray(a, F32))
    return {k: np.stack(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ checking
_REF_CACHE = {}


def probe_reference(R, n, m, family, seed, scale):
    """(batch, fp64 per-ray loss, fp64 gradient, fp64 stage values per ray) of a mode-0 probe batch, computed once."""
    key = (R, n, m, family, seed, scale)
    if key not in _REF_CACHE:
        b = build(R, n, m, family, seed)
        loss, grad = ref_aa(b["s_fin"], b["trans"], b["s_p"], b["c_p"], b["pulse"], scale)
        st = [model(b["s_fin"][r], b["trans"][r], b["s_p"][r], b["c_p"][r], b["pulse"], scale, F64) for r in range(R)]
        _REF_CACHE[key] = (b, loss, grad, st)
    return _REF_CACHE[key]


def check_aa_outputs(ref, scale, loss_rays, grad, what, report=None):
    """What a probe batch asserts of a mode-0 result (the model's or the kernel's), ``ref`` from ``probe_reference``:
    every gradient entry within c_prop_grad u (|G_{j-1}| + |G_j|) scale of the fp64 gradient -- where the hinge is inactive
    on both sides of an edge that bound is 0 and the entry must be exactly 0 -- and every per-ray loss within
    c_prop_ray_loss(m) u of itself."""
    from tests._bounds import U, assert_prop_bound, c_prop_grad, c_prop_ray_loss
    b, loss64, grad64, st = ref
    m = grad64.shape[1] - 1
    gabs = np.stack([np.insert(np.abs(s["G"]), 0, 0.0) + np.append(np.abs(s["G"]), 0.0) for s in st])
    assert_prop_bound(grad, grad64, c_prop_grad() * U * gabs * abs(scale), f"{what} gradient", report)
    assert_prop_bound(loss_rays, loss64, c_prop_ray_loss(m) * U * np.abs(loss64), f"{what} per-ray loss", report)


def pdf_reference(R, n, m, kind, seed, scale):
    key = ("pdf", R, n, m, kind, seed, scale)
    if key not in _REF_CACHE:
        b = build_pdf(R, n, m, kind, seed)
        loss, grad = ref_pdf(b["s_fin"], b["trans"], b["s_p"], b["c_p"], scale)
        st = [model_pdf(b["s_fin"][r], b["trans"][r], b["s_p"][r], b["c_p"][r], scale, F64) for r in range(R)]
        _REF_CACHE[key] = (b, loss, grad, st)
    return _REF_CACHE[key]


def check_pdf_outputs(ref, scale, loss_rays, grad, what, report=None):
    """Mode 1: every gradient entry within c_prop_pdf_grad(hits) u scale sum |g| over the final intervals that scatter into
    it (an entry nothing scatters into is exactly 0), every per-ray loss within c_prop_ray_loss(n) u of itself."""
    from tests._bounds import U, assert_prop_bound, c_prop_pdf_grad, c_prop_ray_loss
    b, loss64, grad64, st = ref
    n = b["trans"].shape[1]
    hits, gabs = np.stack([s["hits"] for s in st]), np.stack([s["gabs"] for s in st])
    assert_prop_bound(grad, grad64, c_prop_pdf_grad(hits) * U * gabs * abs(scale), f"{what} gradient", report)
    assert_prop_bound(loss_rays, loss64, c_prop_ray_loss(n) * U * np.abs(loss64), f"{what} per-ray loss", report)


def realistic_reference(R, n, m, level, seed, scale, oracle):
    """(inputs, pulse, fp64 per-ray loss, fp64 gradient, fp64 stages, bounds per ray) of a realistic batch, computed once."""
    from tests._bounds import prop_aa_bound
    key = ("real", R, n, m, level, seed, scale)
    if key not in _REF_CACHE:
        pulse = float(F32((0.03, 0.003)[level]))
        b = realistic(R, n, m, seed, oracle)
        loss, grad = ref_aa(b["s_fin"], b["trans"], b["s_p"], b["c_p"], pulse, scale)
        st = [model(b["s_fin"][r], b["trans"][r], b["s_p"][r], b["c_p"][r], pulse, scale, F64) for r in range(R)]
        _REF_CACHE[key] = (b, pulse, loss, grad, st, [prop_aa_bound(s, scale) for s in st])
    return _REF_CACHE[key]


def tightness(got, ref, err):
    """(worst err / bound over the entries with a non-zero bound, median bound / |value| over the non-zero values)."""
    got, ref, err = (np.asarray(a, F64).reshape(-1) for a in (got, ref, err))
    pos = err > 0
    worst = float((np.abs(got - ref)[pos] / err[pos]).max()) if pos.any() else 0.0
    nz = ref != 0
    return worst, (float(np.median(err[nz] / np.abs(ref[nz]))) if nz.any() else 0.0)


def check_realistic_outputs(ref, loss_rays, grad, what, report=None):
    """Every gradient entry and every per-ray loss inside its first-order fp64 bound (tests/_bounds.prop_aa_bound): no entry
    excluded, no count of bad entries allowed.  Returns {stage: (worst err / bound, median bound / |value|)}."""
    from tests._bounds import assert_prop_bound
    b, pulse, loss64, grad64, st, bd = ref
    e_grad, e_loss = np.stack([x["grad"] for x in bd]), np.array([x["loss"] for x in bd])
    out = {"gradient": tightness(grad, grad64, e_grad), "per-ray loss": tightness(loss_rays, loss64, e_loss)}
    for k, v in out.items():
        print(f"\n[tightness] {what} {k}: worst err / bound {v[0]:.3g}, median bound / |value| {v[1]:.3e}")
    assert_prop_bound(grad, grad64, e_grad, f"{what} gradient", report)
    assert_prop_bound(loss_rays, loss64, e_loss, f"{what} per-ray loss", report)
    return out


def check_total_and_gradient(s_fin, trans, s_p, c_p, pulse, anti_aliased, scale, upstream, got_loss, got_grad, what):
    """For a caller that sees only the total and the gradient (ops.prop_level_loss on arbitrary small inputs): every
    gradient entry inside its first-order fp64 bound times the (power of two) upstream gradient, the total within the sum
    of the per-ray bounds plus its own rounding.  ``pulse`` is rounded to fp32 as the entry point receives it."""
    from tests._bounds import U, assert_prop_bound, prop_aa_bound, prop_pdf_bound
    a = [np.asarray(x, F32) for x in (s_fin, trans, s_p, c_p)]
    R = a[0].shape[0]
    if anti_aliased:
        pulse = float(F32(pulse))
        loss64, grad64 = ref_aa(*a, pulse, scale)
        bd = [prop_aa_bound(model(a[0][r], a[1][r], a[2][r], a[3][r], pulse, scale, F64), scale) for r in range(R)]
    else:
        loss64, grad64 = ref_pdf(*a, scale)
        bd = [prop_pdf_bound(model_pdf(a[0][r], a[1][r], a[2][r], a[3][r], scale, F64), scale) for r in range(R)]
    e_grad = np.stack([x["grad"] for x in bd]) * abs(upstream)
    w = tightness(got_grad, grad64 * upstream, e_grad)
    print(f"\n[tightness] {what} gradient: worst err / bound {w[0]:.3g}, median bound / |value| {w[1]:.3e}")
    assert_prop_bound(got_grad, grad64 * upstream, e_grad, f"{what} gradient")
    total = float(loss64.sum())
    lim = float(sum(x["loss"] for x in bd)) + U * abs(total)
    assert abs(float(got_loss) - total) <= lim, f"{what}: total {float(got_loss)!r} vs fp64 {total!r}, bound {lim:.3e}"
