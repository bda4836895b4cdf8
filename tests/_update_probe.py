"""Exact probes, fp64 restatements and fp32 operation-order models for the update kernels of csrc/elementwise.hip (test helper,
not a test module): emer_adam_step (adam_kernel and adam_scalar_kernel), emer_contract_bwd, emer_flow_warp_fwd / bwd and
emer_cast_f32_f16.

``restate_*`` evaluate the reference expressions in fp64 from the fp32 inputs and return every intermediate the bounds of
tests/_bounds.py (``adam_bounds``, ``contract_bwd_bounds``, ``flow_warp_bwd_bounds``) need:

* torch.optim.Adam with L2 weight decay (builders.py:50-60) on grad * grad_scale.  Hyperparameters are the c_float values
  the ABI receives; bc1 = 1 - b1^step and bc2_sqrt = sqrt(1 - b2^step) are formed in double, as the host does.
* the gradient of contract() (nerf_utils.py:13-28) under the selector of radiance_field.py:294-299.  The branch decisions --
  inside / outside, mag < 1, the arg-max axis k -- are taken from the fp32 forward model (``model_contract_fwd``, held bit
  for bit to the oracle's contraction, as the kernel's forward is), so no entry has to be excluded: next to a decision
  boundary the two branches agree to within the propagated error (f = 1 and df = 0 at mag = 1), and a point the fp32
  forward puts outside has a gradient of exactly 0.
  TIE CONVENTION: k is the FIRST strict maximum of |u_d| (the kernel's loop); torch's amax backward splits the gradient
  evenly among tied axes.  The random families exclude |u_a| == |u_b| (in fp32) by construction; the exact probes tie only
  below mag < 1, where k is not used.
* the warped query points of radiance_field.py:567-580 and their gradient with respect to the flow.

Exact probes are operands chosen so that every intermediate of the kernel is exactly representable in fp32: a correct
kernel returns the fp64 result bit for bit.  The builders prove that from the fp64 side (``_all_exact``: every intermediate
on a coarse dyadic grid, quotients and roots checked by multiplying back) and tests/test_update_bounds_cpu.py repeats it
for Adam with rationals.  ``model_*`` restate each kernel in fp32 in its own operation order; ``mut`` selects one of
``MUTANTS``.  Unmutated they pass every probe; each mutant fails a probe of the family named for it.
"""
import ctypes
import math

import numpy as np

from tests._bounds import U, adam_bounds, assert_err_bound, contract_bwd_bounds, flow_warp_bwd_bounds
from tests._head_probe import assert_exact

F32, F64 = np.float32, np.float64
SENTINEL = 0x7FC0DEAD          # fp32 NaN with a payload no arithmetic produces
SENTINEL_F16 = 0x7EAD          # the same for a half
GUARD = 9                      # floats / halves in front of and behind every buffer a kernel writes
STREAM_THREADS = 2048 * 256    # stream_blocks() of csrc/elementwise.hip caps every streaming grid at 2048 blocks of 256 threads


def _a(x):
    return np.asarray(x, F64)


def _f(x):
    return np.ascontiguousarray(x, F32)


def cf(x) -> float:
    """x as the c_float the ABI passes, widened back to double."""
    return float(ctypes.c_float(x).value)


def sentinel(shape) -> np.ndarray:
    return np.full(shape, SENTINEL, np.uint32).view(F32)


def is_sentinel(x) -> bool:
    x = np.ascontiguousarray(x)
    if x.dtype == np.float16:
        return bool((x.view(np.uint16) == SENTINEL_F16).all())
    return bool((x.astype(F32, copy=False).view(np.uint32) == SENTINEL).all())


def _all_exact(what, q, lim, **vals):
    """Every value is a multiple of 2^-q below 2^lim (q + lim <= 53: sums and products of such values are exact in fp64) and
    representable in fp32."""
    for k, v in vals.items():
        v = _a(v)
        s = v * 2.0 ** q
        assert np.all(s == np.round(s)) and np.all(np.abs(v) < 2.0 ** lim), f"{what}: {k} leaves the 2^-{q} grid (probe broken)"
        assert np.array_equal(v.astype(F32).astype(F64), v), f"{what}: {k} is not representable in fp32 (probe broken)"


# ======================================================================================================================== Adam
ADAM_HP = dict(lr=0.01, b1=0.9, b2=0.99, eps=1e-15, wd=1e-5, gs=1.0 / 1024, step=1)      # builders.py:54-60, the trainer's grad scale
ADAM_EXACT_HP = dict(lr=2.0 ** -6, b1=0.5, b2=0.75, eps=2.0 ** -12, wd=2.0 ** -3, gs=2.0 ** -10, step=1)
ADAM_EXACT_VARIANTS = {"base": {}, "wd0": dict(wd=0.0), "gs1": dict(gs=1.0)}
ADAM_STEPS = (1, 7, 25000)
PRODUCT_FLOOR = 2.0 ** -40     # every non-zero |g gs| and |wd p| of the main random block: (1 - b2) gi^2 >= 2^-87 stays normal


def adam_consts(hp: dict) -> dict:
    c = {k: cf(hp[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gs")}
    c["step"] = int(hp["step"])
    c["bc1"] = 1.0 - c["b1"] ** c["step"]
    c["bc2_sqrt"] = math.sqrt(1.0 - c["b2"] ** c["step"])
    c["step_size"] = c["lr"] / c["bc1"]
    return c


def restate_adam(p, g, m, v, hp: dict) -> dict:
    """One torch.optim.Adam step (weight_decay as L2, no amsgrad) on grad = g gs, in fp64."""
    c = adam_consts(hp)
    p, g, m, v = _a(p), _a(g), _a(m), _a(v)
    st = dict(c=c, g_gs=g * c["gs"], wd_p=c["wd"] * p)
    st["gi"] = st["g_gs"] + st["wd_p"]
    st["d"] = st["gi"] - m
    st["m1"] = m + st["d"] * (1.0 - c["b1"])
    st["v_b2"] = v * c["b2"]
    st["g2"] = (1.0 - c["b2"]) * st["gi"] * st["gi"]
    st["v1"] = st["v_b2"] + st["g2"]
    st["s"] = np.sqrt(st["v1"])
    st["s_bc"] = st["s"] / c["bc2_sqrt"]
    st["denom"] = st["s_bc"] + c["eps"]
    st["r"] = st["m1"] / st["denom"]
    st["upd"] = c["step_size"] * st["r"]
    st["p1"] = p - st["upd"]
    return st


def build_adam_exact(n: int, variant: str = "base", seed: int = 0) -> dict:
    """Rows whose m', v' and p' are exact: b1 = 1/2, b2 = 3/4, step = 1 (bc1 = bc2_sqrt = 1/2), lr = 2^-6, eps = 2^-12,
    wd = 2^-3, gs = 2^-10 (``variant``: wd = 0 / gs = 1 instead).  S = s 2^-6, gi = +-S, den = 2 S + 2^-12,
    m = 2 k den - gi, v = S^2, p = j 2^-3, g = (gi - wd p) / gs:  m' = k den, v' = S^2, sqrt v' / bc2_sqrt + eps = den,
    m' / den = k and p' = j 2^-3 - k 2^-5."""
    hp = dict(ADAM_EXACT_HP, **ADAM_EXACT_VARIANTS[variant])
    rng = np.random.default_rng(4100 + 7 * n + seed + len(variant))
    s, k, j = rng.integers(1, 64, n), rng.integers(-63, 64, n), rng.integers(-32, 33, n)
    S = s * 2.0 ** -6
    gi = S * rng.choice(np.array([-1.0, 1.0]), n)
    den = 2 * S + 2.0 ** -12
    m, v, p = 2 * k * den - gi, S * S, j * 2.0 ** -3
    g = (gi - hp["wd"] * p) / hp["gs"]
    st = restate_adam(p, g, m, v, hp)
    what = f"adam exact probe ({variant})"
    _all_exact(what, 24, 20, p=p, g=g, m=m, v=v, **{x: st[x] for x in ("g_gs", "wd_p", "gi", "d", "m1", "v_b2", "g2", "v1", "s", "s_bc", "denom", "r", "upd", "p1")})
    assert np.array_equal(st["s"] * st["s"], st["v1"]) and np.array_equal(st["r"] * st["denom"], st["m1"]), f"{what}: root or quotient inexact"
    assert np.array_equal(st["m1"], k * den) and np.array_equal(st["v1"], S * S) and np.array_equal(st["p1"], p - k * 2.0 ** -5)
    return dict(exact=True, hp=hp, n=n, p=_f(p), g=_f(g), m=_f(m), v=_f(v), st=st)


def build_adam_random(n: int, hp: dict, seed: int = 0) -> dict:
    """p ~ N 10^U(-4, 1), g gs ~ N 10^U(-6, 2), m ~ N 10^U(-6, 0), v ~ |N| 10^U(-12, 0); 10 % g = 0, 5 % m = v = 0; and an
    eps block (10 %): g = m = v = 0 with |p| in [1e-11, 1e-8], where for wd = 1e-5 sqrt(v') is comparable with eps = 1e-15.
    Every non-zero |g gs| and |wd p| of the main block is at least PRODUCT_FLOOR (magnitudes are clamped from below), and the
    eps block keeps (1 - b2) (wd p)^2 >= 1e-34: no product leaves the normal range; flushed or kept subnormals are not what
    this family tests."""
    rng = np.random.default_rng(5200 + n + seed)
    c = adam_consts(hp)

    def mag(lo, hi, floor):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)
        return np.where(x < 0, -1.0, 1.0) * np.maximum(np.abs(x), floor)

    p = mag(-4, 1, 1e-6)                              # wd p >= 1e-11 > 2^-40
    g = mag(-6, 2, 1e-11) / c["gs"]                   # g gs >= 1e-11 > 2^-40
    m = mag(-6, 0, 1e-20)
    v = np.abs(mag(-12, 0, 1e-30))
    r = rng.random(n)
    g = np.where((r >= 0.1) & (r < 0.2), 0.0, g)
    zero = (r >= 0.2) & (r < 0.25)
    m, v = np.where(zero, 0.0, m), np.where(zero, 0.0, v)
    epsb = r < 0.1
    pe = 10.0 ** rng.uniform(-11, -8, n) * rng.choice(np.array([-1.0, 1.0]), n)
    p, g, m, v = np.where(epsb, pe, p), np.where(epsb, 0.0, g), np.where(epsb, 0.0, m), np.where(epsb, 0.0, v)
    p, g, m, v = _f(p), _f(g), _f(m), _f(v)
    st = restate_adam(p, g, m, v, hp)
    main = ~epsb
    for x in (st["g_gs"][main], st["wd_p"][main]):
        assert (np.abs(x[x != 0]) >= PRODUCT_FLOOR).all()
    return dict(exact=False, hp=hp, n=n, p=p, g=g, m=m, v=v, st=st, eps_block=epsb)


def check_adam(b: dict, p, m, v, what: str, report: dict = None):
    """m', v', p' as the kernel (or a model) left them: bit for bit on an exact probe, inside adam_bounds otherwise."""
    st = b["st"]
    if b["exact"]:
        for name, got, key in (("m", m, "m1"), ("v", v, "v1"), ("p", p, "p1")):
            assert_exact(f"{what} {name}'", got, st[key], None, 1.0, report)
        return
    bd = adam_bounds(st)
    for name, got, key in (("m", m, "m1"), ("v", v, "v1"), ("p", p, "p1")):
        assert np.isfinite(bd[name]).all()
        assert_err_bound(got, st[key], bd[name], f"{what} {name}'", report)


def adam_split(n: int, off):
    """(head, n4, tail0) of adam_kernel for a slice that starts ``off`` floats behind a 16-byte boundary."""
    head = min((4 - off % 4) % 4, n)
    n4 = (n - head) // 4
    return head, n4, head + 4 * n4


def model_adam(p, g, m, v, hp: dict, off=0, mut: str = ""):
    """(p', m', v') in fp32 in the kernel's order.  ``off``: the slice's phase (head / body / tail split of adam_kernel), or None
    for adam_scalar_kernel, which has no split."""
    c = adam_consts(hp)
    lr, b1, b2, eps, wd, gs = (F32(c[k]) for k in ("lr", "b1", "b2", "eps", "wd", "gs"))
    step = c["step"] - (1 if mut == "step_minus_1" else 0)
    if mut == "betas_exchanged":
        b1, b2 = b2, b1
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    bc1f, bc2s = F32(bc1), F32(math.sqrt(bc2))
    if mut == "bc1_missing":
        bc1f = F32(1)
    if mut == "bc2_missing":
        bc2s = F32(1)
    if mut == "bc2_not_rooted":
        bc2s = F32(bc2)
    if mut == "eps_1e-8":
        eps = F32(1e-8)
    one = F32(1)
    with np.errstate(all="ignore"):
        step_size = lr / bc1f

        def upd(p, g, m, v):
            gi = g if mut == "gs_ignored" else g * gs
            if wd != 0:
                if mut == "gs_after_decay":
                    gi = (g + wd * p) * gs
                elif mut not in ("decay_dropped", "decay_decoupled"):
                    gi = gi + wd * p
            m1 = m + (gi - m) * (b1 if mut == "b1_for_1_minus_b1" else one - b1)
            v1 = v * b2 + ((one - b2) * gi if mut == "g_for_g_squared" else ((one - b2) * gi) * gi)
            if mut == "eps_inside_root":
                den = np.sqrt(v1 + eps) / bc2s
            elif mut == "eps_before_division":
                den = (np.sqrt(v1) + eps) / bc2s
            else:
                den = np.sqrt(v1) / bc2s + eps
            pp = p - (lr * wd) * p if (mut == "decay_decoupled" and wd != 0) else p
            p1 = pp - step_size * ((m if mut == "p_from_old_m" else m1) / den)
            return p1, (m if mut == "m_not_stored" else m1), (v if mut == "v_not_stored" else v1)

        p, g, m, v = _f(p), _f(g), _f(m), _f(v)
        p1, m1, v1 = upd(p, g, m, v)
        if off is not None:
            n = p.size
            head, n4, tail0 = adam_split(n, off)
            if mut == "head_first_skipped" and head > 0:
                p1[0], m1[0], v1[0] = p[0], m[0], v[0]
            if mut == "tail_last_skipped" and n > tail0:
                p1[-1], m1[-1], v1[-1] = p[-1], m[-1], v[-1]
            if mut == "body_vector_twice" and n4 > 0:
                s = slice(head, head + 4)
                p1[s], m1[s], v1[s] = upd(p1[s], g[s], m1[s], v1[s])
    return p1, m1, v1


# ================================================================================================================= contraction
AABB_TRAIN = np.array([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0], F32)      # the trainer's box: widths 100, 80, 20
AABB_EXACT = np.array([-8.0, -4.0, 0.0, 8.0, 4.0, 4.0], F32)           # power-of-two widths 16, 8, 4


def model_contract_fwd(pos, aabb, unbounded) -> dict:
    """contract_point of csrc/contract.h in fp32: the contracted point (zeroed outside) and the decisions the gradient shares
    with it: inside, mag >= 1 (``ge1``) and the arg-max axis k (first strict maximum)."""
    pos, aabb = _f(pos).reshape(-1, 3), _f(aabb).reshape(-1)
    lo, hi = aabb[:3], aabb[3:]
    with np.errstate(all="ignore"):
        v = (pos - lo) / (hi - lo)
        d = dict(ge1=np.zeros(pos.shape[0], bool), k=np.zeros(pos.shape[0], np.int64))
        if unbounded:
            u = v * F32(2) - F32(1)
            au = np.abs(u)
            mag = au.max(1)
            ge1 = ~(mag < 1)
            s = F32(2) - F32(1) / mag
            c = np.where(ge1[:, None], s[:, None] * (u / mag[:, None]), u)
            v = c / F32(4) + F32(0.5)
            d.update(ge1=ge1, k=np.argmax(au, 1), u=u, mag=mag)
        inside = ((v > 0) & (v < 1)).all(1)
        d.update(inside=inside, out=np.where(inside[:, None], v, v * F32(0)).astype(F32))
    return d


def has_tie(dec: dict) -> np.ndarray:
    """Rows whose largest |u_d| is reached on two axes in fp32 (the arg-max of the gradient is then a convention)."""
    au = np.sort(np.abs(dec["u"]), 1)
    return au[:, 2] == au[:, 1]


def restate_contract_bwd(pos, aabb, unbounded, g, dec: dict, e_p=0.0, e_g=0.0) -> dict:
    """d loss / d pos for g = d loss / d contracted, in fp64, with the branch decisions of ``dec`` (module docstring).
    ``pos`` / ``g`` may be fp64 values that carry the errors e_p / e_g against what the kernel holds (the flow warp)."""
    p, g, aabb = _a(pos).reshape(-1, 3), _a(g).reshape(-1, 3), _a(_f(aabb)).reshape(-1)
    lo, hi = aabb[:3], aabb[3:]
    w = hi - lo
    inside = dec["inside"]
    st = dict(unbounded=bool(unbounded), inside=inside, w=w, g=g, e_p=e_p, e_g=e_g)
    if not unbounded:
        st["out"] = np.where(inside[:, None], g / w, 0.0)
        return st
    k, ge1 = dec["k"], dec["ge1"]
    a = p - lo
    b = a / w
    u = 2.0 * b - 1.0
    uk = np.take_along_axis(u, k[:, None], 1)[:, 0]
    mag = np.where(ge1, np.abs(uk), 1.0)           # (unused below 1: f = 1, df = 0 there)
    sgn = np.where(uk >= 0, 1.0, -1.0)
    g4 = g / 4.0
    inv = 1.0 / mag
    f = 2.0 * inv - inv * inv
    df = -2.0 * inv * inv + 2.0 * inv * inv * inv
    t = u * g4
    dot = t.sum(1)
    term = sgn * df * dot
    onk = np.arange(3)[None, :] == k[:, None]
    gu = np.where(ge1[:, None], f[:, None] * g4 + np.where(onk, term[:, None], 0.0), g4)
    st.update(a=a, b=b, u=u, k=k, ge1=ge1, mag=mag, inv=inv, f=f, df=df, g4=g4, t=t, dot=dot, term=term, gu=gu,
              out=np.where(inside[:, None], gu * 2.0 / w, 0.0))
    return st


def model_contract_bwd(pos, aabb, unbounded, g, mut: str = "") -> np.ndarray:
    """contract_point_bwd of csrc/elementwise.hip in fp32, operation by operation."""
    pos, g, aabb = _f(pos).reshape(-1, 3), _f(g).reshape(-1, 3), _f(aabb).reshape(-1)
    lo, hi = aabb[:3], aabb[3:]
    w = hi - lo
    dec = model_contract_fwd(pos, aabb, unbounded)
    inside = np.ones_like(dec["inside"]) if mut == "inside_ignored" else dec["inside"]
    with np.errstate(all="ignore"):
        if unbounded or mut == "bounded_contracts":
            u = (pos - lo) / w * F32(2) - F32(1)
            au = np.abs(u)
            mag = au.max(1)
            k = np.zeros(pos.shape[0], np.int64) if mut == "k_fixed_0" else np.argmax(au, 1)
            ge1 = ~(mag < 1)
            g4 = g / F32(4)
            inv = F32(1) / mag
            f = F32(2) * inv - inv * inv
            df = (F32(-2) * inv) * inv + ((F32(2) * inv) * inv) * inv
            if mut == "df_wrong_sign":
                df = -df
            gd = g if mut == "dot_before_quarter" else g4
            dot = (u[:, 0] * gd[:, 0] + u[:, 1] * gd[:, 1]) + u[:, 2] * gd[:, 2]
            uk = np.take_along_axis(u, k[:, None], 1)[:, 0]
            sgn = np.ones_like(uk) if mut == "sgn_dropped" else np.where(uk >= 0, F32(1), F32(-1))
            term = np.zeros_like(dot) if mut == "delta_term_dropped" else (sgn * df) * dot
            onk = np.arange(3)[None, :] == k[:, None]
            gu = f[:, None] * g4 + np.where(onk, term[:, None], F32(0))
            g = np.where(ge1[:, None], gu, g4)
            if mut != "times_2_missing":
                g = g * F32(2)
        out = g / (np.roll(w, 1) if mut == "wrong_axis_width" else w)
        return np.where(inside[:, None], out, F32(0)).astype(F32)


def _lattice(N: int, rng, first: int = 7):
    """u [N, 3] on the 2^-3 lattice: row i (counted from ``first``) has max |u| < 1 (ties and zeros allowed), == 1, 2, 4 or 8
    by i % 5, reached on axis (i // 5) % 3 with the sign (i // 15) % 2; the other two coordinates are strictly smaller."""
    i = np.arange(N) + first
    sel, k, neg = i % 5, (i // 5) % 3, (i // 15) % 2 == 1
    mag = np.array([1.0, 1.0, 2.0, 4.0, 8.0])[sel]
    lim = (mag * 8).astype(np.int64)
    u = rng.integers(-lim[:, None] + 1, lim[:, None], size=(N, 3)) / 8.0
    big = sel > 0
    uk = np.where(neg, -mag, mag)
    onk = (np.arange(3)[None, :] == k[:, None]) & big[:, None]
    return np.where(onk, uk[:, None], u)


def build_contract_exact(N: int, unbounded: bool, seed: int = 0) -> dict:
    """Points of the lattice in the box AABB_EXACT, g on 2^-2 in [-2, 2]: every intermediate of the gradient is exact.
    Unbounded: all three axes as arg-max with both signs at mag in {1 (f = 1, df = 0), 2, 4, 8}, and mag < 1.  Bounded: the
    mag == 1 rows lie on a face and the larger ones outside (gradient exactly +0), the others inside."""
    rng = np.random.default_rng(6300 + N + seed + int(unbounded))
    u = _lattice(N, rng)
    lo, w = _a(AABB_EXACT[:3]), _a(AABB_EXACT[3:]) - _a(AABB_EXACT[:3])
    pos = lo + (u + 1.0) / 2.0 * w
    g = rng.integers(-8, 9, size=(N, 3)) / 4.0
    b = dict(exact=True, N=N, unbounded=bool(unbounded), aabb=AABB_EXACT, pos=_f(pos), g=_f(g))
    dec = model_contract_fwd(b["pos"], AABB_EXACT, unbounded)
    st = restate_contract_bwd(b["pos"], AABB_EXACT, unbounded, b["g"], dec)
    what = f"contract exact probe (unbounded={unbounded})"
    _all_exact(what, 24, 8, pos=pos, g=g, **{x: st[x] for x in ("a", "b", "u", "inv", "f", "df", "g4", "t", "dot", "term", "gu", "out") if x in st})
    if unbounded:
        assert np.array_equal(st["u"], u) and np.array_equal(dec["u"], u.astype(F32)) and np.array_equal(st["inv"] * st["mag"], np.ones(N))
        assert not (has_tie(dec) & dec["ge1"]).any()
        assert dec["inside"].all()
    else:
        assert np.array_equal(dec["inside"], (np.abs(u) < 1).all(1))
    b["st"] = st
    return b


def contract_points_random(N: int, aabb, rng) -> np.ndarray:
    """Positions around ``aabb``: a broad cloud (inside and up to four widths outside), 1/8 of them within 1e-3 of the box
    centre, 1/8 within 1e-4 (relative to the width) of a face, a few far away; no arg-max ties in fp32."""
    aabb = _a(aabb)
    lo, w = aabb[:3], aabb[3:] - aabb[:3]
    ctr = lo + w / 2
    pos = ctr + (rng.random((N, 3)) - 0.5) * w * 4.0
    r = rng.random(N)
    near_c = r < 0.125
    pos = np.where(near_c[:, None], ctr + rng.uniform(-1e-3, 1e-3, (N, 3)), pos)
    face = (r >= 0.125) & (r < 0.25)
    inner = ctr + (rng.random((N, 3)) - 0.5) * w * 0.9
    ax, side = rng.integers(0, 3, N), rng.integers(0, 2, N)
    onax = np.arange(3)[None, :] == ax[:, None]
    fpos = (lo + side[:, None] * w) + rng.uniform(-1e-4, 1e-4, (N, 1)) * w
    pos = np.where(face[:, None], np.where(onax, fpos, inner), pos)
    far = (r >= 0.25) & (r < 0.27)
    pos = np.where(far[:, None], ctr + rng.standard_normal((N, 3)) * 1e5, pos)
    pos = _f(pos)
    for _ in range(8):
        tie = has_tie(model_contract_fwd(pos, aabb, True))
        if not tie.any():
            break
        pos[tie, 0] = pos[tie, 0] * F32(1.0009765625) + F32(0.01)
    assert not has_tie(model_contract_fwd(pos, aabb, True)).any()
    return pos


def build_contract_random(N: int, unbounded: bool, seed: int = 0) -> dict:
    rng = np.random.default_rng(6400 + N + seed + int(unbounded))
    pos = contract_points_random(N, AABB_TRAIN, rng)
    g = _f(rng.standard_normal((N, 3)))
    g[rng.random(N) < 0.05] = 0.0
    dec = model_contract_fwd(pos, AABB_TRAIN, unbounded)
    return dict(exact=False, N=N, unbounded=bool(unbounded), aabb=AABB_TRAIN, pos=pos, g=g,
                st=restate_contract_bwd(pos, AABB_TRAIN, unbounded, g, dec))


def check_contract_bwd(b: dict, got, what: str, report: dict = None):
    st = b["st"]
    if b["exact"]:
        assert_exact(f"{what} dpos", got, st["out"], None, 1.0, report)
        z = ~st["inside"]
        assert not np.asarray(got, F32).reshape(-1, 3)[z].view(np.uint32).any(), f"{what}: the gradient of an outside point is not +0"
    else:
        assert_err_bound(got, st["out"], contract_bwd_bounds(st), f"{what} dpos", report)


# =================================================================================================================== flow warp
FLOW_DT = 0.25


def _warp_q(pos, flow, noise, h, mut=""):
    fl = flow[:, 3 * h:3 * h + 3]
    return (pos + fl).astype(F32) if mut == "noise_dropped_in_position" else (pos + fl * noise[:, None]).astype(F32)


def model_flow_warp_fwd(pos, normed, ts, flow, noise, dt, aabb, unbounded, mut: str = ""):
    """(x3 [3 n, 4], x2 [2 n, 4]) of flow_warp_fwd_kernel in fp32."""
    pos, normed, ts, flow, noise = _f(pos).reshape(-1, 3), _f(normed).reshape(-1, 3), _f(ts).reshape(-1), _f(flow).reshape(-1, 6), _f(noise).reshape(-1)
    n = pos.shape[0]
    x3 = np.empty((3 * n, 4), F32)
    x3[:n, :3], x3[:n, 3] = normed, ts
    step = F32(cf(dt)) * noise
    for h in (0, 1):
        q = _warp_q(pos, flow, noise, h, mut)
        tw = np.minimum(np.maximum(ts + step if h == 0 else ts - step, F32(0)), F32(1))
        x3[(h + 1) * n:(h + 2) * n, :3] = model_contract_fwd(q, aabb, unbounded)["out"]
        x3[(h + 1) * n:(h + 2) * n, 3] = tw
    return x3, x3[n:].copy()


def _warp_g(dx3, dx2, n, h, mut=""):
    g = np.zeros((n, 3), F32)
    if dx3 is not None:
        r0 = (h if mut == "dx3_rows_h" else h + 1) * n
        g = _f(dx3)[r0:r0 + n, :3]
    if dx2 is not None and mut != "dx2_ignored":
        g = g + _f(dx2)[h * n:(h + 1) * n, :3]
    return g


def model_flow_warp_bwd(pos, flow, noise, aabb, unbounded, dx3, dx2, mut: str = "") -> np.ndarray:
    """dflow [n, 6] of flow_warp_bwd_kernel in fp32."""
    pos, flow, noise = _f(pos).reshape(-1, 3), _f(flow).reshape(-1, 6), _f(noise).reshape(-1)
    n = pos.shape[0]
    out = np.empty((n, 6), F32)
    for h in (0, 1):
        go = model_contract_bwd(_warp_q(pos, flow, noise, h, mut), aabb, unbounded, _warp_g(dx3, dx2, n, h, mut))
        d = 1 - h if mut == "halves_exchanged" else h
        out[:, 3 * d:3 * d + 3] = go if mut == "noise_dropped_in_gradient" else go * noise[:, None]
    return out


def restate_flow_warp_bwd(pos, flow, noise, aabb, unbounded, dx3, dx2, decs=None) -> dict:
    """d loss / d flow in fp64: per half the contraction gradient at q = pos + flow noise of g = dx3[(h + 1) n + i] + dx2[h n + i],
    times the noise.  q and g are exact fp64 values here; what the kernel's fp32 q and g differ from them by goes into the
    bound as e_p and e_g (one product and one sum; one sum)."""
    pos, flow, noise = _f(pos).reshape(-1, 3), _f(flow).reshape(-1, 6), _f(noise).reshape(-1)
    n = pos.shape[0]
    halves = []
    for h in (0, 1):
        fn = _a(flow[:, 3 * h:3 * h + 3]) * _a(noise)[:, None]
        q64 = _a(pos) + fn
        e_q = U * np.abs(fn) + U * np.abs(q64)
        g3 = None if dx3 is None else _a(dx3)[(h + 1) * n:(h + 2) * n, :3]
        g2 = None if dx2 is None else _a(dx2)[h * n:(h + 1) * n, :3]
        g64 = g3 + g2 if (g3 is not None and g2 is not None) else (g3 if g3 is not None else g2)
        e_g = U * np.abs(g64) if (g3 is not None and g2 is not None) else np.zeros_like(g64)
        dec = decs[h] if decs is not None else model_contract_fwd(_warp_q(pos, flow, noise, h), aabb, unbounded)
        halves.append(restate_contract_bwd(q64, aabb, unbounded, g64, dec, e_p=e_q, e_g=e_g))
    return dict(halves=halves, noise=_a(noise), dflow=np.concatenate([h["out"] * _a(noise)[:, None] for h in halves], 1))


FLOW_CONSUMERS = ("dx3", "dx2", "both")


def build_flow(N: int, unbounded: bool, exact: bool, seed: int = 0) -> dict:
    """Inputs of the flow warp and both consumers' gradients.  exact: q = pos + flow noise is a lattice point of
    ``build_contract_exact`` (flow on 2^-2, noise in {0, 1/2, 1}), dx3 and dx2 on 2^-2, t on 2^-3 and dt = 1/4, so that
    t +- dt noise falls below 0, inside and above 1.  Random: the trainer's box, noise in [0, 1) with 1/8 exactly 0,
    t in {0, 1/9 .. 1}: both clamps bind on some rows."""
    rng = np.random.default_rng(7500 + N + seed + 2 * int(unbounded) + int(exact))
    if exact:
        aabb = AABB_EXACT
        lo, w = _a(aabb[:3]), _a(aabb[3:]) - _a(aabb[:3])
        noise = np.array([0.0, 0.5, 1.0])[(np.arange(N) + 1) % 3]
        flow = rng.integers(-16, 17, size=(N, 6)) / 4.0
        q0, q1 = (lo + (_lattice(N, rng, first) + 1.0) / 2.0 * w for first in (7, 11))
        pos = q0 - flow[:, :3] * noise[:, None]
        flow[:, 3:] = np.where(noise[:, None] != 0, (q1 - pos) / np.where(noise == 0, 1.0, noise)[:, None], flow[:, 3:])
        ts = rng.integers(0, 9, N) / 8.0
        dx3, dx2 = rng.integers(-8, 9, size=(3 * N, 4)) / 4.0, rng.integers(-8, 9, size=(2 * N, 4)) / 4.0
        _all_exact("flow exact probe", 24, 10, pos=pos, flow=flow, q0=pos + flow[:, :3] * noise[:, None], q1=pos + flow[:, 3:] * noise[:, None])
    else:
        aabb = AABB_TRAIN
        pos = contract_points_random(N, aabb, rng)
        noise = np.where(rng.random(N) < 0.125, 0.0, rng.random(N))
        flow = rng.standard_normal((N, 6)) * 2.0
        ts = rng.integers(0, 10, N) / 9.0
        dx3, dx2 = rng.standard_normal((3 * N, 4)), rng.standard_normal((2 * N, 4))
    b = dict(exact=exact, N=N, unbounded=bool(unbounded), aabb=aabb, pos=_f(pos), flow=_f(flow), noise=_f(noise), ts=_f(ts), dt=FLOW_DT,
             dx3=_f(dx3), dx2=_f(dx2))
    b["normed"] = model_contract_fwd(b["pos"], aabb, unbounded)["out"]
    if not exact and unbounded:      # no arg-max ties at the warped points either
        for h in (0, 1):
            for _ in range(8):
                tie = has_tie(model_contract_fwd(_warp_q(b["pos"], b["flow"], b["noise"], h), aabb, True))
                if not tie.any():
                    break
                b["flow"][tie, 3 * h] += F32(0.0625)
                b["noise"][tie] = np.maximum(b["noise"][tie], F32(0.25))
            assert not has_tie(model_contract_fwd(_warp_q(b["pos"], b["flow"], b["noise"], h), aabb, True)).any()
    b["x3"], b["x2"] = model_flow_warp_fwd(b["pos"], b["normed"], b["ts"], b["flow"], b["noise"], b["dt"], aabb, unbounded)
    tw = b["x3"][N:, 3]
    if N >= 30:
        step = b["dt"] * b["noise"]
        assert (b["ts"] + step > 1).any() and (b["ts"] - step < 0).any() and ((tw > 0) & (tw < 1)).any() and (b["noise"] == 0).any(), "clamps not reached"
    b["st"] = {}
    decs = [model_contract_fwd(_warp_q(b["pos"], b["flow"], b["noise"], h), aabb, unbounded) for h in (0, 1)]
    for which in FLOW_CONSUMERS:
        d3, d2 = (b["dx3"] if which != "dx2" else None), (b["dx2"] if which != "dx3" else None)
        st = restate_flow_warp_bwd(b["pos"], b["flow"], b["noise"], aabb, unbounded, d3, d2, decs)
        if exact:
            for h in st["halves"]:
                _all_exact("flow exact probe", 24, 8, **{x: h[x] for x in ("a", "b", "u", "f", "df", "t", "dot", "term", "gu", "out") if x in h})
            _all_exact("flow exact probe", 24, 8, dflow=st["dflow"])
        b["st"][which] = st
    return b


def flow_grads(b: dict, which: str):
    return (b["dx3"] if which != "dx2" else None), (b["dx2"] if which != "dx3" else None)


def check_flow_fwd(b: dict, x3, x2, what: str):
    """Bit for bit against the fp32 model (whose contraction tests/test_update_bounds_cpu.py holds to the oracle's)."""
    for name, got, want in (("x3", x3, b["x3"]), ("x2", x2, b["x2"])):
        got = np.ascontiguousarray(got, F32).reshape(want.shape)
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), f"{what} {name}: {int(bad.sum())} entries differ from the fp32 model; first at {tuple(np.argwhere(bad)[0])}"


def check_flow_bwd(b: dict, which: str, got, what: str, report: dict = None):
    st = b["st"][which]
    if b["exact"]:
        assert_exact(f"{what} dflow ({which})", got, st["dflow"], None, 1.0, report)
    else:
        assert_err_bound(got, st["dflow"], flow_warp_bwd_bounds(st), f"{what} dflow ({which})", report)


# ======================================================================================================================== cast
def cast_sources() -> np.ndarray:
    """fp32 sources of the fp16 cast: every finite half, every midpoint between two adjacent halves (the one between 65504 and
    the overflow threshold 65520 included) and its two fp32 neighbours, both signs; 65504, 65519.996, 65520, +-inf, NaN, +-0;
    the fp32 values around the largest half subnormal (2^-14 - 2^-24) and around half the smallest one (2^-25: the tie between
    0 and 2^-24, and its neighbours)."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(F32)           # +0 .. 65504
    nxt = np.concatenate([h[1:], np.array([65536.0], F32)])
    mid = ((h.astype(F64) + nxt.astype(F64)) / 2).astype(F32)
    assert np.array_equal(mid.astype(F64), (h.astype(F64) + nxt.astype(F64)) / 2)
    pos = np.concatenate([h, mid, np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf))])
    sub = F32(2.0 ** -14 - 2.0 ** -24)
    edge = [65504.0, 65519.996, 65520.0, np.inf, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14]
    for x in (sub, F32(2.0 ** -25), F32(2.0 ** -14), F32(2.0 ** -24)):
        edge += [np.nextafter(x, F32(0)), x, np.nextafter(x, F32(1))]
    pos = np.concatenate([pos, np.array(edge, F32)])
    rng = np.random.default_rng(88)
    src = np.concatenate([pos, -pos, np.array([np.nan, 0.0, -0.0], F32)])
    return _f(src[rng.permutation(src.size)])


def cast_ref(src) -> np.ndarray:
    with np.errstate(over="ignore"):
        return _f(src).astype(np.float16)      # IEEE round to nearest even


def check_cast(src, got, what: str):
    """got: the half buffer (bits) the kernel left for the n sources; NaN compares as NaN, everything else bit for bit."""
    want = cast_ref(src)
    got = np.ascontiguousarray(got).view(np.float16).reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ"
    bad = (got.view(np.uint16) != want.view(np.uint16)) & ~nan
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.size} halves differ; first at {i}: source {_f(src)[i]!r} -> {got[i]!r}, want {want[i]!r}")


def model_cast(buf, start: int, n: int, mut: str = "") -> np.ndarray:
    """The n halves the cast kernel writes for the source buf[start : start + n] (``start`` floats behind a 16-byte boundary:
    the scalar-load path when start % 4 != 0), as uint16 bits in a sentinel-filled array."""
    src = _f(buf)[start:start + n]
    if mut == "unaligned_shifted" and start % 4 != 0:
        src = np.concatenate([_f(buf)[start + 1:start + n], np.zeros(1, F32)])[:n]
    with np.errstate(all="ignore"):
        h = src.astype(np.float16)
        away = np.abs(h.astype(F32)) > np.abs(src)
        down = np.where(away, np.nextafter(h, np.float16(0)), h)       # towards zero
        if mut == "truncation":
            h = down
        elif mut == "ties_away":
            up = np.where(away, h, np.nextafter(h, np.where(src < 0, np.float16(-np.inf), np.float16(np.inf))))
            fin = np.where(np.isinf(up), np.where(src < 0, -65536.0, 65536.0), up.astype(F64))
            tie = (np.abs(src.astype(F64) - down.astype(F64)) == np.abs(fin - src.astype(F64))) & np.isfinite(src) & (down.astype(F64) != src)
            h = np.where(tie, up, h)
        elif mut == "saturation":
            h = np.where(np.isinf(h) & np.isfinite(src), np.where(src < 0, np.float16(-65504), np.float16(65504)), h)
    out = np.full(n, SENTINEL_F16, np.uint16)
    live = n - n % 8 if mut == "tail_dropped" else n
    out[:live] = h.view(np.uint16)[:live]
    return out


# ===================================================================================================================== mutants
# name -> (family whose probes must catch it, what the slip is)
MUTANTS = {
    "decay_dropped": ("adam", "the L2 term wd p is not added to the gradient"),
    "decay_decoupled": ("adam", "AdamW: p (1 - lr wd) instead of the L2 term"),
    "gs_after_decay": ("adam", "grad_scale applied to g + wd p"),
    "gs_ignored": ("adam", "grad_scale not applied"),
    "eps_inside_root": ("adam", "sqrt(v' + eps)"),
    "eps_before_division": ("adam", "(sqrt v' + eps) / bc2_sqrt"),
    "eps_1e-8": ("adam", "torch's default eps instead of the argument"),
    "bc1_missing": ("adam", "step_size = lr"),
    "bc2_missing": ("adam", "sqrt v' not divided by bc2_sqrt"),
    "bc2_not_rooted": ("adam", "sqrt v' divided by bc2"),
    "step_minus_1": ("adam", "bias corrections of step - 1"),
    "betas_exchanged": ("adam", "b1 and b2 exchanged"),
    "b1_for_1_minus_b1": ("adam", "lerp weight b1"),
    "g_for_g_squared": ("adam", "v' from g instead of g^2"),
    "m_not_stored": ("adam", "exp_avg not written back"),
    "v_not_stored": ("adam", "exp_avg_sq not written back"),
    "p_from_old_m": ("adam", "p updated from the old exp_avg"),
    "head_first_skipped": ("adam", "the first head element is not updated"),
    "tail_last_skipped": ("adam", "the last tail element is not updated"),
    "body_vector_twice": ("adam", "the first body vector is updated twice (the update is in place)"),
    "sgn_dropped": ("contract", "the arg-max term without the sign of u_k"),
    "df_wrong_sign": ("contract", "df with the wrong sign"),
    "k_fixed_0": ("contract", "the arg-max term always on axis 0"),
    "delta_term_dropped": ("contract", "the arg-max term dropped"),
    "dot_before_quarter": ("contract", "u . g taken before g / 4"),
    "times_2_missing": ("contract", "the factor 2 of u = 2 v - 1 missing"),
    "wrong_axis_width": ("contract", "divided by the width of another axis"),
    "inside_ignored": ("contract", "the selector ignored: outside points get a gradient"),
    "bounded_contracts": ("contract", "bounded mode applies the contraction's factors"),
    "noise_dropped_in_gradient": ("flow", "dflow without the factor noise"),
    "noise_dropped_in_position": ("flow", "q = pos + flow"),
    "dx2_ignored": ("flow", "the flow table's gradient dx2 not added"),
    "dx3_rows_h": ("flow", "dx3 read at rows h instead of h + 1"),
    "halves_exchanged": ("flow", "the forward and backward halves of dflow exchanged"),
    "truncation": ("cast", "round towards zero"),
    "ties_away": ("cast", "ties rounded away from zero"),
    "tail_dropped": ("cast", "the n % 8 tail is not written"),
    "unaligned_shifted": ("cast", "the scalar-load path reads one float too far"),
    "saturation": ("cast", "overflow saturates at 65504 instead of inf"),
}
