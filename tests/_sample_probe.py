"""Exact probes, fp64 restatements and fp32 operation-order models for the kernels that decide where every sample of a step lands
(test helper, not a test module): emer_importance_sample, emer_importance_sample_points and emer_stot of csrc/sampler.hip,
emer_ray_points of csrc/elementwise.hip, and ray_point / contract_point of csrc/contract.h, which they share.

The models are written from the frozen rule of SURVEY.md A.2 and the reference's Python call sites, not from the kernels or the
C oracle:

* the sampler: u_k = c_first + (k + beta) step with step = (c_last - c_first) / (n + 1), beta = 0.5 or the ray's jitter;
  the bracket is numpy's ``searchsorted(side="right")`` with the two indices clamped separately to [0, m - 1]; a bracket
  narrower than 1e-10 returns the midpoint of its two edges, any other interpolates (u - c_p) ((v_q - v_p) / d) + v_p;
* _transform_stot (nerfacc_prop_net.py:299-339): s_min / s_max are the forward map of the planes, evaluated in fp32 on the
  host (``log`` by the C library's logf, as the host does); t is the inverse map of s s_max + (1 - s) s_min.  torch evaluates
  ``200 / (2 - 2 x)`` as (2 - 2 x).reciprocal() * 200;
* the sample point ((d (t0 + t1)) / 2) + o (render_utils.py:341), its contraction (``_update_probe.model_contract_fwd``, held
  to the oracle there), the per-ray ``times`` column of out_dim = 4 and the world positions;
* the fused kernel's outputs as the composition of the three.

Every model rounds each operation to fp32 and takes ``mut=``, one of ``MUTANTS``.  Exact probes are inputs for which every
intermediate is exactly representable in fp32, so the fp64 evaluation (``restate_*``) is the answer bit for bit whatever the
order or contraction; the builders prove it (``_all_exact`` grids, representability, products and quotients multiplied back).
Random families are compared with the un-mutated model bit for bit: this family's bar is equality, no bound is
involved.  The one exception is the ``log`` map, whose inverse is the library's expf: ``LOG_ULP``.
"""
import ctypes
import ctypes.util

import numpy as np

from tests._head_probe import assert_exact
from tests._update_probe import AABB_EXACT, AABB_TRAIN, _all_exact, cf, is_sentinel, model_contract_fwd  # noqa: F401 (is_sentinel: for the GPU module)

F32, F64 = np.float32, np.float64
STOT_TYPES = {"uniform": 0, "uniform_lindisp": 1, "lindisp": 2, "sqrt": 3, "log": 4, "uniform_lindisp_0": 5}
THRESHOLD = F32(1e-10)
# |expf(x) - exp(x)| of a ``log`` result, in ulps of the result, x the model's (bit-exact) fp32 argument.
#   CPU (glibc expf in the oracle, torch.exp in the recorded fixture): every result is within 1 ulp (as an integer distance
#   of the bit patterns) of the correctly rounded one; tests/test_sample_bounds_cpu.py prints the measured maxima.
#   Device: no document available to this project states the error of the device library's expf, so the bound is the
#   maximum observed on an MI355X on the first run of tests/test_sample_exact_gpu.py -- 0.785 ulp over the 2 x 10^4 arguments
#   of the random family, final rounding included; 93.6 % of the results are the correctly rounded one -- plus 1 ulp
#   (DESIGN 4.4d).  DESIGN 4.4 has an earlier sweep of the same expf over [-100, 0]: 0.836 ulp, also inside this bound.
LOG_ULP_CPU = 1
LOG_ULP_DEVICE_OBSERVED = 0.785
LOG_ULP_DEVICE = LOG_ULP_DEVICE_OBSERVED + 1.0


def _a(x):
    return np.asarray(x, F64)


def _f(x):
    return np.ascontiguousarray(x, F32)


def _repr32(what, **vals):
    for k, v in vals.items():
        v = _a(v)
        with np.errstate(all="ignore"):
            assert np.array_equal(v.astype(F32).astype(F64), v), f"{what}: {k} is not representable in fp32 (probe broken)"


def same_bits(what, got, want, report=None):
    """Bit for bit, every entry; where ``want`` is NaN, ``got`` must be NaN (the class is compared, not the payload)."""
    want = _f(want)
    got = np.ascontiguousarray(got, F32).reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs differ from the model's"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {want.size} entries differ from the fp32 model; first at {i}: got {got[i]!r}, want {want[i]!r}")
    if report is not None:
        report[what] = 1.0          # every entry compared: there is no exclusion


def ulp_distance(got, want64) -> np.ndarray:
    """|got - want| in ulps of fp32(want), want in fp64 (positive, finite, normal)."""
    want64 = _a(want64)
    w32 = want64.astype(F32)
    ulp = _a(np.spacing(np.abs(w32)))
    return np.abs(_a(got) - want64) / ulp


def check_log(what, got, arg, limit, report=None) -> float:
    """A ``log`` result against exp, in fp64, of the model's fp32 argument: at most ``limit`` ulps (the library's error plus the
    half ulp of the final rounding).  Returns the largest distance."""
    want = np.exp(_a(arg))
    with np.errstate(all="ignore"):
        fin = np.isfinite(want.astype(F32)) & (want > 2.0 ** -126)
    assert fin.all(), f"{what}: the family leaves fp32's normal range (probe broken)"
    got = _a(np.ascontiguousarray(got, F32).reshape(np.shape(arg)))
    e = ulp_distance(got, want)
    worst = float(e.max()) if e.size else 0.0
    assert worst <= limit, f"{what}: expf is {worst:.3f} ulp from exp of the fp32 argument (limit {limit})"
    if report is not None:
        report[what] = 1.0
    return worst


# ============================================================================================================== s -> t maps
_libm = None


def _logf(x) -> np.float32:
    """The C library's logf, which the host evaluates the ``log`` planes with."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.logf.restype, _libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    return F32(_libm.logf(ctypes.c_float(float(x))))


def stot_fwd(typ: str, t) -> np.float32:
    """_contract_fn of TRANSFROM_DICT on one plane, in fp32 (the plane is the c_float the ABI receives)."""
    t = F32(cf(t))
    one, two = F32(1), F32(2)
    with np.errstate(all="ignore"):
        if typ == "uniform":
            return t
        if typ == "lindisp":
            return one / t
        if typ == "sqrt":
            return np.sqrt(t)
        if typ == "log":
            return _logf(t)
        if typ == "uniform_lindisp":
            return t / F32(400) if t < F32(200) else one - one / (two * t / F32(200))
        if typ == "uniform_lindisp_0":
            return t / two if t < one else one - one / (two * t)
    raise ValueError(typ)


def stot_arg(typ: str, s, t_min, t_max, mut: str = "") -> np.ndarray:
    """s s_max + (1 - s) s_min in fp32: the argument of the inverse map."""
    s = _f(s)
    s_min, s_max = stot_fwd(typ, t_min), stot_fwd(typ, t_max)
    with np.errstate(all="ignore"):
        if mut == "blend_lerp":
            return s_min + s * (s_max - s_min)
        return s * s_max + (F32(1) - s) * s_min


def stot_inv(typ: str, x, mut: str = "") -> np.ndarray:
    """_icontract_fn in fp32.  ``log``: exp in fp64 rounded once (compare within LOG_ULP_*, never bit for bit)."""
    x = _f(x)
    one, two = F32(1), F32(2)
    with np.errstate(all="ignore"):
        if typ == "uniform":
            return x
        if typ == "lindisp":
            return one / x
        if typ == "sqrt":
            return x * x
        if typ == "log":
            return np.exp(x.astype(F64)).astype(F32)
        low = x <= F32(0.5) if mut == "break_le" else x < F32(0.5)
        if typ == "uniform_lindisp":
            far = F32(200) / (two - two * x) if mut == "one_division" else (one / (two - two * x)) * F32(200)
            return np.where(low, x * F32(400), far).astype(F32)
        if typ == "uniform_lindisp_0":
            return np.where(low, two * x, one / (two - two * x)).astype(F32)
    raise ValueError(typ)


def model_stot(typ: str, s, t_min, t_max, mut: str = "") -> np.ndarray:
    return stot_inv(typ, stot_arg(typ, s, t_min, t_max, mut), mut)


def restate_stot(typ: str, s, t_min, t_max) -> dict:
    """The same map in fp64 with every intermediate (exact probes only: ``log`` planes must be 1)."""
    s, t_min, t_max = _a(s), cf(t_min), cf(t_max)

    def fwd(t):
        with np.errstate(all="ignore"):
            if typ == "uniform":
                return t
            if typ == "lindisp":
                return 1.0 / t
            if typ == "sqrt":
                return float(np.sqrt(t))
            if typ == "log":
                assert t == 1.0
                return 0.0
            if typ == "uniform_lindisp":
                return t / 400.0 if t < 200.0 else 1.0 - 1.0 / (2.0 * t / 200.0)
            return t / 2.0 if t < 1.0 else 1.0 - 1.0 / (2.0 * t)

    st = dict(s_min=fwd(t_min), s_max=fwd(t_max))
    with np.errstate(all="ignore"):
        st["a"], st["om"] = s * st["s_max"], 1.0 - s
        st["b"] = st["om"] * st["s_min"]
        x = st["x"] = st["a"] + st["b"]
        if typ == "uniform":
            t = x
        elif typ == "lindisp":
            t = 1.0 / x
            ok = np.isfinite(t)
            assert np.array_equal((t * x)[ok], np.ones(int(ok.sum()))), "stot exact probe: 1 / x is not exact"
        elif typ == "sqrt":
            t = x * x
        elif typ == "log":
            assert not x.any()
            t = np.ones_like(x)
        else:
            den = st["den"] = 2.0 - 2.0 * x
            far = x >= 0.5
            rec = st["rec"] = np.where(far, 1.0 / np.where(far, den, 1.0), 1.0)
            assert np.array_equal(rec * np.where(far, den, 1.0), np.ones_like(x)), "stot exact probe: the reciprocal is not exact"
            t = np.where(far, rec * 200.0, x * 400.0) if typ == "uniform_lindisp" else np.where(far, rec, 2.0 * x)
    st["t"] = t
    return st


def _k64(ks):
    return np.asarray(list(ks), F64) / 64.0


STOT_EXACT = (            # (type, t_min, t_max, s): the planes' images, both products, their sum and the inverse are all exact
    ("uniform", 0.5, 64.0, _k64(range(65))),
    ("uniform_lindisp", 100.0, 400.0, _k64(list(range(33)) + [64])),        # s_min 1/4, s_max 3/4: x < 0.5 | == 0.5 (s = 1/2) | 3/4
    ("uniform_lindisp", 0.0, 200.0, _k64(range(65))),                       # t_max at the forward break: s = 1 reaches x == 0.5
    ("uniform_lindisp", 200.0, 800.0, _k64([0, 64])),                       # t_min at the forward break (s_min = 1/2)
    ("uniform_lindisp", 200.0, 102400.0, _k64([0, 64])),
    ("uniform_lindisp_0", 0.5, 2.0, _k64(list(range(33)) + [64])),
    ("uniform_lindisp_0", 0.0, 1.0, _k64(range(65))),
    ("uniform_lindisp_0", 1.0, 4.0, _k64([0, 64])),                         # t_min at the forward break 1
    ("lindisp", 0.5, 64.0, _k64([0, 64])),
    ("lindisp", 0.5, np.inf, 1.0 - 2.0 ** -np.arange(11.0)),                # s_max = 0: x = 2^(1 - j), and s = 0 -> x = 2
    ("lindisp", 4.0, 0.25, _k64([0, 64])),
    ("sqrt", 4.0, 64.0, _k64(range(65))),
    ("sqrt", 0.0, 1.0, _k64(range(65))),
    ("log", 1.0, 1.0, _k64(range(65))),                                     # x = 0: expf(0) is 1
)


def build_stot_exact():
    out = []
    for typ, t_min, t_max, s in STOT_EXACT:
        st = restate_stot(typ, s, t_min, t_max)
        what = f"stot exact probe {typ} ({t_min}, {t_max})"
        _repr32(what, s=s, **{k: v for k, v in st.items()})
        _all_exact(what, 30, 20, s=s, a=st["a"], om=st["om"], b=st["b"], x=st["x"])
        if typ != "log":     # the fp32 model reaches the same planes (logf(1) = 0 needs no proof)
            assert _a(stot_fwd(typ, t_min)) == st["s_min"] and _a(stot_fwd(typ, t_max)) == st["s_max"], what
        out.append(dict(name=f"stot exact {typ} ({t_min:g}, {t_max:g})", exact=True, typ=typ, planes=(t_min, t_max), s=_f(s), want64=st["t"], x64=st["x"]))
    xs = {b["typ"]: np.concatenate([c["x64"] for c in out if c["typ"] == b["typ"]]) for b in out}
    for typ in ("uniform_lindisp", "uniform_lindisp_0"):
        assert (xs[typ] == 0.5).any() and (xs[typ] < 0.5).any() and (xs[typ] > 0.5).any(), "both sides of the break and the break itself"
    return out


STOT_RANDOM_PLANES = ((0.1, 1000.0), (0.5, 300.0))


def stot_random_s(n: int = 10_000, seed: int = 0) -> np.ndarray:
    """n values of s in [0, 1]: uniform, with 0, 1, 0.5 and the neighbours of 0.5, and a block clustered where the piecewise
    maps' argument crosses 0.5."""
    rng = np.random.default_rng(8100 + seed)
    s = rng.random(n).astype(F32)
    half = F32(0.5)
    s[:8] = [0.0, 1.0, 0.5, np.nextafter(half, F32(0)), np.nextafter(half, F32(1)), 2.0 ** -24, 1.0 - 2.0 ** -24, 0.25]
    return _f(s)


def build_stot_random(n: int = 10_000):
    out = []
    for typ in STOT_TYPES:
        for j, planes in enumerate(STOT_RANDOM_PLANES):
            s = stot_random_s(n, j)
            if typ.startswith("uniform_lindisp"):       # a quarter of the values land within a few ulps of the break x = 0.5
                s_min, s_max = _a(stot_fwd(typ, planes[0])), _a(stot_fwd(typ, planes[1]))
                s_half = (0.5 - s_min) / (s_max - s_min)
                q = n // 4
                s[8:8 + q] = (s_half * (1.0 + np.random.default_rng(j).integers(-40, 41, q) * 2.0 ** -24)).astype(F32)
            out.append(dict(name=f"stot random {typ} ({planes[0]:g}, {planes[1]:g})", exact=False, typ=typ, planes=planes, s=s,
                            arg=stot_arg(typ, s, *planes), want=model_stot(typ, s, *planes)))
    return out


def check_stot(b: dict, got, what: str, report: dict = None, log_limit: float = LOG_ULP_CPU + 0.5):
    if b["exact"]:
        assert_exact(what, got, b["want64"], None, 1.0, report)
    elif b["typ"] == "log":
        check_log(what, got, b["arg"], log_limit, report)
    else:
        same_bits(what, got, b["want"], report)


# ================================================================================================================= the sampler
def _bracket(c, u, m, mut=""):
    p = np.stack([np.searchsorted(c[r], u[r], side="left" if mut == "lower_bound" else "right") for r in range(c.shape[0])])
    if mut == "joint_clamp":
        p0 = np.clip(p - 1, 0, m - 2)
        return p0, p0 + 1
    return np.clip(p - 1, 0, m - 1), np.clip(p, 0, m - 1)


def model_sampler(vals, cdfs, n: int, jitter=None, mut: str = "") -> np.ndarray:
    """The n + 1 edges per ray in fp32."""
    v, c = _f(vals), _f(cdfs)
    R, m = c.shape
    c0, cl = c[:, :1], c[:, -1:]
    N = F32(n + 1)
    with np.errstate(all="ignore"):
        step = (cl - c0) * (F32(1) / N) if mut == "step_reciprocal" else (cl - c0) / N
        beta = np.full((R, 1), 0.0 if mut == "beta_default_0" else 0.5, F32) if jitter is None else _f(jitter).reshape(R, 1)
        k = np.arange(n + 1, dtype=F32)[None, :]
        u = (c0 + k * step) + beta * step if mut == "u_split" else c0 + (k + beta) * step
        p0, p1 = _bracket(c, u, m, mut)
        cp, cq, vp, vq = (np.take_along_axis(a, i, 1) for a, i in ((c, p0), (c, p1), (v, p0), (v, p1)))
        d = cq - cp
        thr = F32(1e-9) if mut == "thr_1e-9" else F32(0) if mut == "thr_0" else THRESHOLD
        mid = (vp + vq) * F32(0.5)
        slope = (vq - vp) / d
        if mut == "interp_fma":
            lin = ((u - cp).astype(F64) * slope.astype(F64) + vp.astype(F64)).astype(F32)
        else:
            lin = (u - cp) * slope + vp
        return np.where(d < thr, mid, lin).astype(F32)


def model_sample(b: dict, mut: str = "") -> dict:
    """Edges s, edge times t and the interval form (starts, ends) of a build."""
    s = model_sampler(b["vals"], b["cdfs"], b["n"], b["jitter"], mut)
    t_min, t_max, typ = b["stot"]
    t = model_stot(typ, s, t_min, t_max, mut)
    return dict(s=s, t=t, ts=np.ascontiguousarray(t[:, :-1]), te=np.ascontiguousarray(t[:, :-1] if mut == "ends_from_k" else t[:, 1:]))


def restate_sampler(vals, cdfs, n: int, beta) -> dict:
    """The frozen rule in fp64 with its intermediates (exact probes only); beta [R]."""
    v, c = _a(_f(vals)), _a(_f(cdfs))
    R, m = c.shape
    c0, cl = c[:, :1], c[:, -1:]
    span = cl - c0
    step = span / (n + 1)
    kb = np.arange(n + 1.0)[None, :] + _a(beta).reshape(R, 1)
    ks = kb * step
    u = c0 + ks
    p0, p1 = _bracket(c, u, m)
    cp, cq, vp, vq = (np.take_along_axis(a, i, 1) for a, i in ((c, p0), (c, p1), (v, p0), (v, p1)))
    d, dv, off = cq - cp, vq - vp, u - cp
    flat = d < float(THRESHOLD)
    with np.errstate(all="ignore"):
        slope = np.where(flat, 0.0, dv / np.where(flat, 1.0, d))
    prod = off * slope
    s = np.where(flat, (vp + vq) * 0.5, prod + vp)
    return dict(span=span, step=step, kb=kb, ks=ks, u=u, d=d, dv=dv, off=np.where(flat, 0.0, off), slope=slope, prod=prod, vsum=vp + vq, s=s, flat=flat, p0=p0, p1=p1)


UNIFORM_EXACT = (0.25, 2.0, "uniform")      # t = 2 s + (1 - s) / 4: exact for the probes' s


def _finish_exact(name, vals, cdfs, n, jitter, extra=None):
    vals, cdfs = _f(vals), _f(cdfs)
    R = vals.shape[0]
    beta = np.full(R, 0.5) if jitter is None else _a(jitter)
    st = restate_sampler(vals, cdfs, n, beta)
    what = f"sampler exact probe {name}"
    _repr32(what, **{k: st[k] for k in ("span", "step", "kb", "ks", "u", "d", "dv", "off", "slope", "prod", "vsum", "s")})
    _all_exact(what, 38, 2, span=st["span"], step=st["step"], ks=st["ks"], u=st["u"], d=st["d"], off=st["off"])
    _all_exact(what, 26, 4, dv=st["dv"], prod=st["prod"], vsum=st["vsum"], s=st["s"])
    assert np.array_equal(st["step"] * (n + 1), st["span"]) and np.array_equal(st["slope"] * st["d"], np.where(st["flat"], 0.0, st["dv"])), f"{what}: a quotient is inexact"
    tt = restate_stot("uniform", st["s"], UNIFORM_EXACT[0], UNIFORM_EXACT[1])
    _repr32(what, **tt)
    _all_exact(what, 26, 4, a=tt["a"], om=tt["om"], b=tt["b"], x=tt["x"])
    b = dict(name=name, exact=True, vals=vals, cdfs=cdfs, n=n, jitter=None if jitter is None else _f(jitter), stot=UNIFORM_EXACT, st=st,
             want64=dict(s=st["s"], t=tt["t"], ts=tt["t"][:, :-1], te=tt["t"][:, 1:]))
    b.update(extra or {})
    b["want"] = model_sample(b)
    return b


def _pow2_partition(total: int, parts: int, rng) -> list:
    w = [total]
    while len(w) < parts:
        i = int(rng.choice([j for j, x in enumerate(w) if x > 1]))
        x = w.pop(i)
        w += [x // 2, x // 2]
    return w


def build_dyadic(m: int, n: int, jitter_kind: str, R: int = 5, seed: int = 0) -> dict:
    """CDF values c_first + A_j delta with widths A_{j+1} - A_j powers of two (or 0) that sum to 4 (n + 1), n + 1 a power of two:
    step = 4 delta, and u_k lies on the delta grid for beta in {0.5, 0.25, 0}.  Edge distances are powers of two, so every
    slope is one.  Odd rows have c_first = 1/8 and c_last = 5/8."""
    N = n + 1
    assert N & (N - 1) == 0
    rng = np.random.default_rng(9000 + 131 * m + n + seed)
    total = 4 * N
    zeros = max((m - 1) // 8, m - 1 - total)
    vals, cdfs = np.zeros((R, m)), np.zeros((R, m))
    for r in range(R):
        w = np.array(_pow2_partition(total, m - 1 - zeros, rng) + [0] * zeros, F64)
        w = w[rng.permutation(m - 1)]
        c0, span = (0.125, 0.5) if r % 2 else (0.0, 1.0)
        cdfs[r] = c0 + np.concatenate([[0.0], np.cumsum(w)]) * (span / total)
        dv = 2.0 ** -rng.integers(7, 11, m - 1).astype(F64)
        vals[r] = (0.0625 if r % 3 == 1 else 0.0) + np.concatenate([[0.0], np.cumsum(dv)])
    jitter = None if jitter_kind == "default" else np.array([0.25, 0.0, 0.5])[np.arange(R) % 3]
    b = _finish_exact(f"dyadic m={m} n={n} jitter={jitter_kind}", vals, cdfs, n, jitter)
    assert (b["cdfs"][1::2, 0] != 0).all() and (b["cdfs"][1::2, -1] != 1).all()
    return b


def build_ties() -> dict:
    """beta = 0 and n + 1 = 8: u_k = c_first + k span / 8 meets interior CDF values exactly, among them a run of three equal ones
    (u_4): the upper-bound search steps over the run to the bracket behind it; a lower-bound search stops in front of it."""
    c = np.array([0.0, 0.25, 0.5, 0.5, 0.5, 0.75, 1.0])
    v = np.array([0.0, 0.0625, 0.125, 0.1875, 0.25, 0.5, 1.0])
    cdfs = np.stack([c, c / 2 + 0.25, c, c / 4])
    vals = np.stack([v, v + 0.125, v * 2, v])
    b = _finish_exact("ties", vals, cdfs, 7, np.zeros(4))
    st = b["st"]
    tie = (st["u"][:, :, None] == _a(b["cdfs"])[:, None, 1:-1]).any(-1)
    assert tie.sum() >= 12 and np.array_equal(st["s"][0, 4], 0.25), "the tie rows do not tie"
    return b


def build_threshold() -> dict:
    """CDF values that are multiples of e = 2^-34: brackets of width 2 e = 2^-33 (> 1e-10: interpolate), e (< 1e-10: midpoint)
    and 4 e in one ray, sampled with step = e at beta = 0.5, 0.25 and 0; an all-equal CDF (step = 0: every u equals c, the
    search runs off the row, both indices clamp to m - 1, the bracket has width exactly 0 and every edge is v[m - 1]); an
    all-zero CDF."""
    e = 2.0 ** -34
    c = np.array([0.0, 2.0, 3.0, 3.0, 4.0, 8.0]) * e
    v = np.array([0.0, 0.25, 0.5, 0.625, 0.75, 1.0])
    cdfs = np.stack([c, c, c, np.full(6, _a(F32(0.3))), np.zeros(6)])
    vals = np.stack([v, v, v, v + 0.5, v])
    b = _finish_exact("threshold", vals, cdfs, 7, np.array([0.5, 0.25, 0.0, 0.5, 0.25]))
    st = b["st"]
    assert 2 * e > float(THRESHOLD) > e
    assert ((st["d"][:3] == 2 * e) & ~st["flat"][:3]).any() and ((st["d"][:3] == e) & st["flat"][:3]).any() and (st["d"][3:] == 0).all()
    assert np.array_equal(st["s"][3], np.full(8, 1.5)) and np.array_equal(st["s"][4], np.ones(8)), "an all-equal CDF returns v[m - 1]"
    return b


def build_end_clamp() -> dict:
    """tests/test_oracle_cpu._end_clamp_case: beta = 1 - 2^-24, so (n + beta) rounds to n + 1 and u_n == c_last.  Not an exact
    probe (the CDF is not dyadic): compared with the model, and its last edge is pinned to v[m - 1]."""
    from tests.test_oracle_cpu import _end_clamp_case
    vals, cdf, n, jit = _end_clamp_case()
    b = dict(name="end clamp", exact=False, vals=_f(vals.numpy()), cdfs=_f(cdf.numpy()), n=n, jitter=_f(jit.numpy()), stot=(0.1, 1000.0, "uniform_lindisp"))
    b["pin_last"] = b["vals"][:, -1].copy()
    b["want"] = model_sample(b)
    return b


JITTERS = ("none", "uniform", "edge")
_RANDOM_STOT = ((0.1, 1000.0, "uniform_lindisp"), (0.5, 300.0, "uniform_lindisp_0"), (0.5, 300.0, "lindisp"), (0.25, 100.0, "sqrt"), (0.1, 1000.0, "uniform"))


def build_random(R: int, m: int, n: int, jitter_kind: str, seed: int = 0) -> dict:
    """Peaky histograms w^4; ray 0 half flat, ray 1 all-zero weights, ray 2 rescaled to 0.6 c + 0.1, ray 3 with its mass in one
    bin (as far as R reaches), rays 4, 6, ... rescaled by a random factor and offset.  Jitter: none | uniform | a vector that contains 0 and 1 - 2^-24."""
    rng = np.random.default_rng(9500 + 1009 * R + 31 * m + n + seed + JITTERS.index(jitter_kind))
    w = (rng.random((R, m - 1)) ** 4).astype(F32)
    w[0, :(m - 1) // 2] = 0
    if R > 1:
        w[1] = 0
    if R > 3:
        w[3] = 0
        w[3, int(rng.integers(0, m - 1))] = 1
    c = np.concatenate([np.zeros((R, 1), F32), np.cumsum(w, 1, dtype=F32)], 1)
    c = (c / np.maximum(c[:, -1:], F32(1e-12))).astype(F32)
    if R > 2:
        c[2] = c[2] * F32(0.6) + F32(0.1)
    for r in range(4, R, 2):      # further rows with c_last - c_first != 1: the step is a quotient that a reciprocal multiply misses
        c[r] = c[r] * F32(rng.uniform(0.3, 0.9)) + F32(rng.uniform(0.0, 0.1))
    assert (np.diff(c, axis=1) >= 0).all()
    vals = np.sort(rng.random((R, m)).astype(F32), 1)
    jitter = None
    if jitter_kind != "none":
        jitter = rng.random(R).astype(F32)
        if jitter_kind == "edge":
            jitter[0] = 0.0
            jitter[-1] = F32(1.0) - F32(2.0 ** -24)
            if R > 2:
                jitter[1] = F32(1.0) - F32(2.0 ** -24)       # on the all-zero ray as well
    b = dict(name=f"random R={R} m={m} n={n} jitter={jitter_kind}", exact=False, vals=vals, cdfs=c, n=n, jitter=jitter,
             stot=_RANDOM_STOT[(R + m + n + seed) % len(_RANDOM_STOT)])
    b["want"] = model_sample(b)
    return b


def check_sample(b: dict, got: dict, what: str, report: dict = None):
    """got: whichever of s, t, ts, te a form of the kernel (or a model) produced."""
    for k, x in got.items():
        if b["exact"]:
            assert_exact(f"{what} {k}", x, b["want64"][k], None, 1.0, report)
        same_bits(f"{what} {k} (model)", x, b["want"][k], None if b["exact"] else report)
    if "pin_last" in b and "s" in got:
        assert np.array_equal(np.asarray(got["s"]).reshape(b["vals"].shape[0], -1)[:, -1], b["pin_last"]), f"{what}: u >= c_last must return the last edge"


def edges_sorted_and_inside(b: dict, s) -> bool:
    s = np.asarray(s, F32).reshape(b["vals"].shape[0], -1)
    return bool((np.diff(s, axis=1) >= 0).all() and (s >= b["vals"][:, :1]).all() and (s <= b["vals"][:, -1:]).all())


# =================================================================================================================== ray points
def model_ray_points(origins, dirs, ts, te, aabb, unbounded, times=None, mut: str = "") -> dict:
    """normed [R, S, 3 | 4] and positions [R, S, 3] in fp32: ((d (t0 + t1)) / 2) + o, then the contraction."""
    o, d, ts, te = _f(origins).reshape(-1, 3), _f(dirs).reshape(-1, 3), _f(ts), _f(te)
    R, S = ts.shape
    i = np.arange(R * S)
    r = (i % S) % R if mut == "ray_index_mod" else i // S
    t0, t1 = ts.reshape(-1, 1), te.reshape(-1, 1)
    two = F32(2)
    with np.errstate(all="ignore"):
        if mut == "midpoint_offset":
            p = d[r] * (t0 + (t1 - t0) / two) + o[r]
        elif mut == "point_fma":
            p = (d[r].astype(F64) * ((t0 + t1) / two).astype(F64) + o[r].astype(F64)).astype(F32)
        else:
            p = (d[r] * (t0 + t1)) / two + o[r]
        dec = model_contract_fwd(p, aabb, unbounded)
    q = dec["out"]
    if mut == "outside_assigned_0":
        q = np.where(dec["inside"][:, None], q, F32(0)).astype(F32)
    if times is not None:
        tm = _f(times).reshape(-1)
        col = tm[i % tm.size] if mut == "times_per_sample" else tm[r]
        q = np.concatenate([q, col[:, None]], 1)
    return dict(normed=q.reshape(R, S, -1), pos=_f(p).reshape(R, S, 3))


def model_sample_points(b: dict, mut: str = "") -> dict:
    """The fused kernel: the interval form of the sampler, then the points of its intervals."""
    out = model_sample(b, mut)
    g = b["geo"]
    out.pop("t")
    out.update(model_ray_points(g["o"], g["d"], out["ts"], out["te"], g["aabb"], g["unbounded"], None, mut))
    return out


POINT_T = np.array([0.25, 0.5, 1.0, 1.5, 2.0, 4.0, 8.0, 16.0])       # |u_a| = t / 2: below 1, exactly 1, 2, 4, 8
POINT_DT = np.array([0.125, 0.25, 0.0, 0.0625])


def build_points_exact(R: int, S: int, unbounded: bool, seed: int = 0) -> dict:
    """Dyadic origins, directions and times in the box AABB_EXACT (power-of-two widths).  In contracted coordinates u = 2 v - 1
    a ray runs u(t) = u0 + g t with u0_a = 0 and g_a = +-1/2 on its dominant axis a = r % 3 and |u0|, |g t| small on the other
    two; the interval midpoints cycle through POINT_T, so max |u| is below 1, exactly 1 (on a face: outside for the bounded
    selector), 2, 4 and 8, each a power of two: 1 / mag, v / mag and (2 - 1 / mag) (v / mag) are exact."""
    rng = np.random.default_rng(9700 + 17 * R + S + seed + int(unbounded))
    lo, w = _a(AABB_EXACT[:3]), _a(AABB_EXACT[3:]) - _a(AABB_EXACT[:3])
    a = np.arange(R) % 3
    onax = np.arange(3)[None, :] == a[:, None]
    sign = np.where((np.arange(R) // 3) % 2 == 1, -1.0, 1.0)
    u0 = np.where(onax, 0.0, rng.integers(-2, 3, (R, 3)) / 8.0)
    g = np.where(onax, sign[:, None] * 0.5, rng.integers(-4, 5, (R, 3)) / 32.0)
    o, d = lo + (u0 + 1.0) / 2.0 * w, g * w / 2.0
    j = np.arange(R)[:, None] * 3 + np.arange(S)[None, :]
    tm, dt = POINT_T[j % POINT_T.size], POINT_DT[(j // POINT_T.size) % POINT_DT.size]
    ts, te = tm - dt, tm + dt
    times = np.arange(R) / 64.0 + 0.125
    # fp64 restatement with every intermediate
    tsum = ts + te
    prod = d[:, None, :] * tsum[..., None]
    pos = prod / 2.0 + o[:, None, :]
    v = (pos - lo) / w
    st = dict(tsum=tsum, prod=prod, pos=pos, dlo=pos - lo, v=v)
    if unbounded:
        u = 2.0 * v - 1.0
        mag = np.abs(u).max(-1, keepdims=True)
        far = mag >= 1.0
        inv = 1.0 / np.where(far, mag, 1.0)
        um = u * inv
        f = 2.0 - inv
        c = np.where(far, f * um, u)
        assert np.array_equal(inv * np.where(far, mag, 1.0), np.ones_like(mag)), "points exact probe: 1 / mag is inexact"
        assert np.array_equal((u / np.where(far, mag, 1.0)) * np.where(far, mag, 1.0), u), "points exact probe: v / mag is inexact"
        v = c / 4.0 + 0.5
        st.update(u=u, mag=mag, inv=inv, um=um, f=f, c=c, vc=v)
        assert np.array_equal(u, u0[:, None, :] + g[:, None, :] * (tsum / 2.0)[..., None])
        if R * S >= 8:
            assert all((mag == x).any() for x in (1.0, 2.0)) and (mag < 1.0).any(), "mag exactly 1 and exactly 2 are reached"
    inside = ((v > 0) & (v < 1)).all(-1)
    normed = np.where(inside[..., None], v, 0.0)
    what = f"points exact probe R={R} S={S} unbounded={unbounded}"
    _all_exact(what, 24, 8, o=o, d=d, ts=ts, te=te, normed=normed, **st)
    if not unbounded and R * S >= 8:
        assert (~inside).any() and inside.any() and ((v == 0) | (v == 1)).any(), "points on a face"
    return dict(name=f"points exact R={R} S={S} unbounded={unbounded}", exact=True, R=R, S=S, unbounded=bool(unbounded), aabb=AABB_EXACT, o=_f(o), d=_f(d),
                ts=_f(ts), te=_f(te), times=_f(times), want64=dict(normed=normed, pos=pos))


def build_points_random(R: int, S: int, unbounded: bool, seed: int = 0) -> dict:
    """Origins in the trainer's box, unit directions, sorted interval edges in [0.1, 300]: the rays leave the box (mag = 1) on
    the way.  Every fourth ray has its edges scaled by 1000 (far outside); the last ray ends at t = inf (R >= 3): its last
    points are +-inf and their contraction NaN."""
    rng = np.random.default_rng(9800 + 17 * R + S + seed + int(unbounded))
    o = rng.random((R, 3)) * np.array([60.0, 4.0, 1.0]) + np.array([0.0, -2.0, 1.5])
    d = np.array([1.0, 0.0, 0.0]) + 0.6 * rng.standard_normal((R, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    edges = np.sort(rng.random((R, S + 1)) * 300 + 0.1, 1)
    edges[1::4] *= 1000.0
    edges = _f(edges)
    ts, te = edges[:, :-1].copy(), edges[:, 1:].copy()
    if R >= 3:
        te[-1, -1] = np.inf
        if S > 1:
            ts[-1, -1] = te[-1, -2] = np.inf
        assert (_f(d)[-1] != 0).all()
    b = dict(name=f"points random R={R} S={S} unbounded={unbounded}", exact=False, R=R, S=S, unbounded=bool(unbounded), aabb=AABB_TRAIN, o=_f(o), d=_f(d),
             ts=ts, te=te, times=_f(rng.random(R)))
    b["want3"] = model_ray_points(b["o"], b["d"], ts, te, b["aabb"], unbounded)
    b["want4"] = model_ray_points(b["o"], b["d"], ts, te, b["aabb"], unbounded, b["times"])
    if unbounded and R * S >= 64:
        dec = model_contract_fwd(b["want3"]["pos"].reshape(-1, 3), b["aabb"], True)
        assert dec["ge1"].any() and (~dec["ge1"]).any(), "both sides of mag = 1"
    return b


def check_points(b: dict, got: dict, what: str, report: dict = None, out_dim: int = 3):
    """got: normed [R, S, out_dim] and, if asked for, pos [R, S, 3]."""
    R, S = b["R"], b["S"]
    normed = np.asarray(got["normed"], F32).reshape(R, S, out_dim)
    if out_dim == 4:
        assert np.array_equal(normed[..., 3].view(np.uint32), np.broadcast_to(b["times"][:, None], (R, S)).view(np.uint32)), f"{what}: the times column is not the ray's time"
    if b["exact"]:
        assert_exact(f"{what} normed", normed[..., :3], b["want64"]["normed"], None, 1.0, report)
        if got.get("pos") is not None:
            assert_exact(f"{what} pos", got["pos"], b["want64"]["pos"], None, 1.0, report)
        return
    want = b["want4" if out_dim == 4 else "want3"]
    same_bits(f"{what} normed", normed, want["normed"], report)
    if got.get("pos") is not None:
        same_bits(f"{what} pos", got["pos"], want["pos"], report)


def attach_geometry(b: dict, unbounded: bool, seed: int = 0) -> dict:
    """Origins, directions and a box for the fused kernel on the rays of a sampler build (``geo``), and the model's outputs."""
    R = b["vals"].shape[0]
    rng = np.random.default_rng(9900 + R + seed)
    if b["exact"]:      # dyadic geometry; the points of these rays are held to the model (their t is exact, the contraction need not be)
        o, d, aabb = rng.integers(-16, 17, (R, 3)) / 4.0, rng.integers(-4, 5, (R, 3)) / 4.0, AABB_EXACT
    else:
        o = rng.random((R, 3)) * 60 - 10
        d = rng.standard_normal((R, 3))
        d, aabb = d / np.linalg.norm(d, axis=1, keepdims=True), AABB_TRAIN
    b = dict(b, geo=dict(o=_f(o), d=_f(d), aabb=aabb, unbounded=bool(unbounded)))
    b["want_points"] = model_sample_points(b)
    return b


def check_sample_points(b: dict, got: dict, what: str, report: dict = None):
    """Every output of the fused kernel (or of model_sample_points under a mutant): s, ts, te as check_sample holds them, normed
    and pos bit for bit against the model."""
    check_sample(b, {k: got[k] for k in ("s", "ts", "te")}, what, report)
    for k in ("normed", "pos"):
        if got.get(k) is not None:
            same_bits(f"{what} {k}", got[k], b["want_points"][k], report)


# ====================================================================================================================== mutants
# name -> (family whose probes must catch it, what the slip is)
MUTANTS = {
    "lower_bound": ("sampler", "lower-bound search: the first j with c[j] >= u"),
    "joint_clamp": ("sampler", "the lower index clamped to [0, m - 2] and the upper one taken as the next"),
    "thr_1e-9": ("sampler", "the flat-bracket threshold 1e-9"),
    "thr_0": ("sampler", "the flat-bracket threshold 0"),
    "step_reciprocal": ("sampler", "step as a multiply by the reciprocal of n + 1"),
    "u_split": ("sampler", "u = (c0 + k step) + beta step"),
    "beta_default_0": ("sampler", "beta defaults to 0 without a jitter tensor"),
    "interp_fma": ("sampler", "the interpolation as one fused multiply-add"),
    "ends_from_k": ("sampler", "interval ends taken from edge k instead of k + 1"),
    "blend_lerp": ("stot", "the blend as s_min + s (s_max - s_min)"),
    "one_division": ("stot", "200 / (2 - 2 s) as one division"),
    "midpoint_offset": ("points", "the midpoint as t0 + (t1 - t0) / 2"),
    "point_fma": ("points", "o + d t as one fused multiply-add"),
    "ray_index_mod": ("points", "the ray index as i % S"),
    "times_per_sample": ("points", "the times column taken per sample instead of per ray"),
    "outside_assigned_0": ("points", "the outside selector as an assignment of 0: loses the NaN (and the sign of -0)"),
}
# Slips no input can show: the two branches of both piecewise inverses agree bit for bit at the break (2 x = 1 / (2 - 2 x) = 1 and
# 400 x = (1 / (2 - 2 x)) 200 = 200 at x = 0.5), so testing the break with <= computes the same function.
EQUIVALENT = {"break_le": ("stot", "the break of the inverse at 0.5 tested with <=")}
