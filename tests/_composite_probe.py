"""Probes and fp64 restatement of the compositing kernels (csrc/composite.hip and the ray epilogue of csrc/rayloss.hip), and
the checks the CPU and GPU tests share.  Test helper, not a test module: tests/test_composite_exact_gpu.py holds the kernels
to it, tests/test_composite_bounds_cpu.py the numpy model of tests/_composite_model.py.

* ``ref_*``: the operations restated in plain float64 numpy from the formulas in the kernels' header comments (cumsum, exp,
  the closed-form reverse mode).  Every function returns the outputs together with the abs-sums the bounds of
  tests/_bounds.py need.
* ``*_probe``: inputs on which every fp32 operation of the kernels is exact, so the kernels must reproduce the fp64 values
  as numbers, entry by entry, in any summation order (only the sign of a zero is not held).  Wall probes: edges on multiples
  of 0.25, sigma 0 or 128 / dt, so sigma dt is 0 or 128, exp(-0) = 1 and expf(-128) = 0 in fp32: T, alpha and w are 0 or 1.
  Dyadic probes: small multiples of powers of two whose products and sums stay below 2^24 units.  The builders assert
  these preconditions.
* ``check_*``: what a set of outputs must satisfy on a probe (exact) or on arbitrary inputs (inside the bounds).
"""
import numpy as np

from tests import _bounds as B
from tests._composite_model import EPS, F32, F64, W

SPECIAL_WSUM = [F32(0), np.nextafter(EPS, F32(0)), EPS, np.nextafter(EPS, F32(1)), F32(1), np.nextafter(F32(1), F32(2))]

WALL_S = (1, 2, 63, 64, 65, 128, 129, 200, 4096)
WALL_R = (1, 4, 5, 13)
ACC_C = (None, 1, 2, 3, 4, 5, 6, 7, 8, 9, 64, 65, 100, 129)
ACC_S = (1, 63, 64, 65, 129)
ACC_R = (1, 5)
BLEND_S = (1, 63, 64, 65, 130)
WIDE_S = (1, 3, 4, 5, 7, 8, 9, 12, 13, 129)
WIDE_C = (1, 63, 64, 65, 130)
WIDE_R = (1, 3)
WIDE_CAP = (4099, 129, 1)            # R S = 528771 > 16384 workgroups x 4 waves x 2 quads x 4 samples; S % 4 = 1
REAL_SHAPES = ((5, 1), (13, 64), (7, 130), (5, 333), (3, 4096))
REAL_SEED = 2024                     # no ray of REAL_SHAPES has a cumsum of w within its bound of 0.5 (asserted on the CPU)
BLEND_KEYS = ("acc", "acs", "d_w", "d_sig", "d_ss", "d_sd", "d_rs", "d_rd", "d_sh")
WIDE_KEYS = ("acc", "d_w", "d_sig", "d_ss", "d_sd", "d_fs", "d_fd")
EXP128 = 2.0 ** -100                 # what float64 keeps of exp(-128) = 2.6e-56 times any probe value stays far below this


# --------------------------------------------------------------------------------------------------- fp64 restatement
def _rcumsum(x):
    return np.cumsum(x[:, ::-1], 1)[:, ::-1]


def _shift_left(x):
    """x[:, i] <- x[:, i + 1], 0 at the end (inclusive suffix sum -> strictly-later sum)."""
    return np.concatenate([x[:, 1:], np.zeros_like(x[:, :1])], 1)


def ref_render(ts, te, sg):
    """Forward in float64: x = sigma dt, T_i = exp(-sum_{j<i} x_j), alpha = 1 - exp(-x), w = T alpha, cdfs = 1 - [T, 0],
    stats = (sum w, sum w mid, mid of the first sample whose inclusive cumsum of w reaches 0.5, else of the last)."""
    ts, te, sg = (np.asarray(x, F64) for x in (ts, te, sg))
    R, S = sg.shape
    dts, mid = te - ts, (ts + te) / 2
    x = sg * dts
    cum = np.cumsum(x, 1)
    excl = np.concatenate([np.zeros((R, 1)), cum[:, :-1]], 1)
    with np.errstate(under="ignore"):
        T, e = np.exp(-excl), np.exp(-x)
        al = -np.expm1(-x)
    w = T * al
    cw = np.cumsum(w, 1)
    idx = np.minimum((cw < 0.5).sum(1), S - 1)
    # (sum w telescopes to 1 - T_S: taken in closed form, so that it never rounds above 1)
    stats = np.stack([-np.expm1(-cum[:, -1]), (w * mid).sum(1), mid[np.arange(R), idx], np.zeros(R)], 1)
    cdfs = np.concatenate([1 - T, np.ones((R, 1))], 1)
    return dict(x=x, A=np.cumsum(np.abs(x), 1), T=T, e=e, al=al, w=w, cw=cw, mid=mid, dts=dts, cdfs=cdfs, stats=stats,
                weights=w, trans=T, alphas=al, t_mid=mid, t_dist=dts)


def ref_render_bwd(rf, gw, gT, gA):
    """d_sigma_i = dt_i (gw_i T_{i+1} - sum_{k>i} (gw_k w_k + gT_k T_k) + gA_i exp(-x_i)) with gw the whole gradient that
    reaches w_i.  Also returns the pieces the bound needs."""
    T, e, w = rf["T"], rf["e"], rf["w"]
    P, Q = gw * T * e, gA * e
    term = gw * w + gT * T
    later = _shift_left(_rcumsum(term))
    return dict(d_sigma=rf["dts"] * (P - later + Q), P=P, Q=Q, gw=gw, gT=gT, gA=gA)


def ref_epilogue(stats, acc=None, sky=None, do=None, dd=None, drgb=None, passes=None):
    """opacity = clamp(sum w, 1e-6f, 1), depth = sum(w mid) / opacity, rgb = acc + sky (1 - opacity), and the reverse mode
    (the clamp passes the gradient on its closed range).  ``passes``: the clamp branch per ray, where the caller knows which
    one the kernel took (``clamp_branch``); default: the branch of the fp64 sum."""
    st = np.asarray(stats, F64)
    R = st.shape[0]
    lo = F64(EPS)
    o = np.clip(st[:, 0], lo, 1.0)
    passes = ((st[:, 0] >= lo) & (st[:, 0] <= 1.0)) if passes is None else np.asarray(passes, bool)
    out = dict(opacity=o, depth=st[:, 1] / o, median=st[:, 2], passes=passes, stats=st)
    acc = None if acc is None else np.asarray(acc, F64)
    sky = None if (sky is None or acc is None) else np.asarray(sky, F64)
    out.update(acc=acc, sky=sky)
    if acc is not None:
        out["rgb"] = acc if sky is None else acc + sky * (1 - o)[:, None]
    do = np.zeros(R) if do is None else np.asarray(do, F64).reshape(R)
    dd = np.zeros(R) if dd is None else np.asarray(dd, F64).reshape(R)
    t_dep = dd * st[:, 1] / (o * o)
    go, go_abs = do - t_dep, np.abs(do) + np.abs(t_dep)
    if drgb is not None and sky is not None:
        g = np.asarray(drgb, F64).reshape(R, 3)
        go, go_abs = go - (g * sky).sum(1), go_abs + np.abs(g * sky).sum(1)
        out["d_sky"], out["g_abs"] = g * (1 - o)[:, None], np.abs(g)
    out.update(go=go, go_abs=go_abs, g0=np.where(out["passes"], go, 0.0), g1=dd / o, dd=dd)
    return out


def ref_render_all(p):
    """render_weights on ``p``: forward, d_sigma and the bound's pieces."""
    rf = ref_render(p["ts"], p["te"], p["sg"])
    S = rf["x"].shape[1]
    d = {k: np.asarray(p[k], F64) for k in ("dW", "dT", "dA", "dC", "dS")}
    g1m = d["dS"][:, 1:2] * rf["mid"]
    gw = d["dW"] + d["dS"][:, 0:1] + g1m
    rb = ref_render_bwd(rf, gw, d["dT"] - d["dC"][:, :S], d["dA"])
    rb.update(gw_abs=np.abs(d["dW"]) + np.abs(d["dS"][:, 0:1]) + np.abs(g1m), gT_abs=np.abs(d["dT"]) + np.abs(d["dC"][:, :S]),
              e_g0=np.zeros(len(gw)), e_g1=np.zeros(len(gw)))
    return rf, rb


def clamp_branch(rf, e_sum, wsum_k):
    """The branch of the clamp's gradient the kernel took, from its own fp32 sum w.  It may differ from the branch of the
    fp64 sum only on a ray whose fp64 sum is within its error bound of a clamp bound (a saturated ray's fp32 sum rounds
    above 1 about as often as not); anywhere else a difference is an error."""
    wk = np.asarray(wsum_k, F32).reshape(-1)
    x = rf["stats"][:, 0]
    took, ref = (wk >= EPS) & (wk <= F32(1)), (x >= F64(EPS)) & (x <= 1.0)
    near = (np.abs(x - F64(EPS)) <= e_sum) | (np.abs(x - 1.0) <= e_sum)
    bad = (took != ref) & ~near
    assert not bad.any(), f"clamp gradient mask differs on rays {np.flatnonzero(bad)} whose sum w is not within its bound of 1e-6 or 1"
    return took


def ref_composite_all(p, passes=None):
    """composite_rgb on ``p``: render -> accumulate(rgb) -> epilogue and the reverse, in float64 (``passes``: ref_epilogue)."""
    rf = ref_render(p["ts"], p["te"], p["sg"])
    R, S = rf["x"].shape
    rgb = None if p.get("rgb") is None else np.asarray(p["rgb"], F64)
    acc = None if rgb is None else (rf["w"][..., None] * rgb).sum(1)
    ep = ref_epilogue(rf["stats"], acc, p.get("sky"), p.get("d_opa"), p.get("d_dep"), p.get("d_out") if rgb is not None else None, passes)
    dW = np.zeros((R, S)) if p.get("dW") is None else np.asarray(p["dW"], F64)
    dT = np.zeros((R, S)) if p.get("dT") is None else np.asarray(p["dT"], F64)
    g1m = ep["g1"][:, None] * rf["mid"]
    gw, gw_abs = dW + ep["g0"][:, None] + g1m, np.abs(dW) + np.abs(ep["g0"][:, None]) + np.abs(g1m)
    if rgb is not None and p.get("d_out") is not None:
        g = np.asarray(p["d_out"], F64).reshape(R, 1, 3)
        gw, gw_abs = gw + (g * rgb).sum(2), gw_abs + np.abs(g * rgb).sum(2)
        ep["d_rgb"] = rf["w"][..., None] * g
    rb = ref_render_bwd(rf, gw, dT, np.zeros((R, S)))
    rb.update(gw_abs=gw_abs, gT_abs=np.abs(dT))
    ep.update(acc_abs=None if rgb is None else (rf["w"][..., None] * np.abs(rgb)).sum(1))
    return rf, ep, rb


def ref_accumulate(w, v, go):
    """out[r, c] = sum_s w v, d_w = sum_c go v, d_v = w go; with the abs-sums."""
    w, go = np.asarray(w, F64), np.asarray(go, F64)
    if v is None:
        return dict(out=w.sum(1, keepdims=True), out_abs=np.abs(w).sum(1, keepdims=True),
                    d_w=np.broadcast_to(go, w.shape), d_w_abs=np.zeros(w.shape))
    v = np.asarray(v, F64)
    t, gv, d_v = w[..., None] * v, go[:, None, :] * v, w[..., None] * go[:, None, :]
    return dict(out=t.sum(1), out_abs=np.abs(t).sum(1), d_w=gv.sum(2), d_w_abs=np.abs(gv).sum(2), d_v=d_v, d_v_abs=np.abs(d_v))


def ref_blend(p, den=None):
    """a = sigma_s / den, b = sigma_d / den, den = sigma + 1e-6f; rgb = a rgb_s (1 - shadow) + b rgb_d; acc = sum_s w rgb,
    acs = sum_s w shadow^2, and the closed-form gradients.  ``den``: the probes pass the fp32 sum (== sigma there)."""
    def g(k):
        return None if p.get(k) is None else np.asarray(p[k], F64)
    w, sig, ss, sd, rs, rd, sh, g_rgb, g_sh = (g(k) for k in ("w", "sig", "ss", "sd", "rs", "rd", "sh", "g_rgb", "g_sh"))
    inv = 1.0 / (sig + F64(EPS) if den is None else np.asarray(den, F64))
    a, b = ss * inv, sd * inv
    s_ = np.zeros_like(w) if sh is None else sh
    ka = a * (1 - s_)
    t_s, t_d = w[..., None] * ka[..., None] * rs, w[..., None] * b[..., None] * rd
    o = dict(acc=(t_s + t_d).sum(1), acc_abs=(np.abs(t_s) + np.abs(t_d)).sum(1))
    gs = np.zeros(w.shape[0]) if (sh is None or g_sh is None) else g_sh.reshape(-1)
    G = g_rgb[:, None, :]
    gS, gD, gSa, gDa = (G * rs).sum(2), (G * rd).sum(2), np.abs(G * rs).sum(2), np.abs(G * rd).sum(2)
    if sh is not None:
        o["acs"], o["d_sh"] = (w * s_ * s_).sum(1), w * (2 * gs[:, None] * s_ - a * gS)
        o["acs_abs"], o["d_sh_abs"] = np.abs(w * s_ * s_).sum(1), np.abs(w) * (np.abs(2 * gs[:, None] * s_) + np.abs(a) * gSa)
    sh2 = gs[:, None] * s_ * s_
    o["d_w"], o["d_w_abs"] = ka * gS + b * gD + sh2, np.abs(ka) * gSa + np.abs(b) * gDa + np.abs(sh2)
    o["d_rs"], o["d_rd"] = G * (w * ka)[..., None], G * (w * b)[..., None]
    o["d_rs_abs"], o["d_rd_abs"] = np.abs(o["d_rs"]), np.abs(o["d_rd"])
    da, db, daa, dba = w * (1 - s_) * gS, w * gD, np.abs(w * (1 - s_)) * gSa, np.abs(w) * gDa
    o["d_ss"], o["d_sd"], o["d_sig"] = da * inv, db * inv, -(da * ss + db * sd) * inv * inv
    o["d_ss_abs"], o["d_sd_abs"], o["d_sig_abs"] = daa * inv, dba * inv, (daa * np.abs(ss) + dba * np.abs(sd)) * inv * inv
    return o


def ref_blend_wide(p, den=None):
    """acc[r, c] = sum_s w (a feat_s[c] + b feat_d[c]) and its gradients, a and b as in ``ref_blend``."""
    def g(k):
        return np.asarray(p[k], F64)
    w, sig, ss, sd, fs, fd, up = (g(k) for k in ("w", "sig", "ss", "sd", "fs", "fd", "g_acc"))
    inv = 1.0 / (sig + F64(EPS) if den is None else np.asarray(den, F64))
    a, b = ss * inv, sd * inv
    t_s, t_d = (w * a)[..., None] * fs, (w * b)[..., None] * fd
    o = dict(acc=(t_s + t_d).sum(1), acc_abs=(np.abs(t_s) + np.abs(t_d)).sum(1))
    G = up[:, None, :]
    mS, mD, mSa, mDa = (G * fs).sum(2), (G * fd).sum(2), np.abs(G * fs).sum(2), np.abs(G * fd).sum(2)
    o["d_w"], o["d_w_abs"] = a * mS + b * mD, np.abs(a) * mSa + np.abs(b) * mDa
    o["d_fs"], o["d_fd"] = G * (w * a)[..., None], G * (w * b)[..., None]
    o["d_fs_abs"], o["d_fd_abs"] = np.abs(o["d_fs"]), np.abs(o["d_fd"])
    da, db, daa, dba = w * mS, w * mD, np.abs(w) * mSa, np.abs(w) * mDa
    o["d_ss"], o["d_sd"], o["d_sig"] = da * inv, db * inv, -(da * ss + db * sd) * inv * inv
    o["d_ss_abs"], o["d_sd_abs"], o["d_sig_abs"] = daa * inv, dba * inv, (daa * np.abs(ss) + dba * np.abs(sd)) * inv * inv
    return o


# ------------------------------------------------------------------------------------------------------------- probes
def _units(abs_sum, unit, what):
    """Every partial sum of a scan fits 2^24 units of its smallest term: it is exact in any order."""
    assert float(np.max(abs_sum)) / unit < 2.0 ** 24, f"{what}: abs-sum {float(np.max(abs_sum)):g} exceeds 2^24 units of {unit:g}"


def _multiple(x, unit, what):
    q = np.asarray(x, F64) / unit
    assert np.array_equal(q, np.round(q)), f"{what}: not a multiple of {unit:g}"


def _dy(rng, shape, unit, lo, hi):
    """Random multiples of ``unit`` in [lo, hi]."""
    return (rng.integers(int(round(lo / unit)), int(round(hi / unit)) + 1, size=shape) * unit).astype(F32)


def wall_configs(S):
    """Wall positions for a ray of S samples: none, {0, 1, 62, 63, 64, 65, 127, 128, S - 1} where they exist, and two walls
    in two different chunks."""
    single = sorted({q for q in (0, 1, 62, 63, 64, 65, 127, 128, S - 1) if 0 <= q < S})
    cfg = [()] + [(q,) for q in single]
    if S > W:
        cfg += [(1, S - 1), (63, 64)]
    if S > 2 * W:
        cfg += [(65, S - 1)]
    return cfg


def wall_probe(R, S, rot=0, seed=0):
    """R rays of S samples; ray r takes wall configuration (rot + r) mod n.  Keys: ts, te, sg; upstream gradients dW, dT, dA,
    dC [R, S + 1], dS [R, 4] (columns 2, 3 carry no gradient and hold 7) for render_weights; rgb, sky, d_out, d_opa, d_dep
    for composite_rgb; walls (per ray)."""
    rng = np.random.default_rng(1000 * S + 10 * R + seed)
    cfg = wall_configs(S)
    walls = [cfg[(rot + r) % len(cfg)] for r in range(R)]
    dts = (0.25 * 2.0 ** rng.integers(0, 3, size=(R, S))).astype(F32)
    start = _dy(rng, (R, 1), 0.25, 0.25, 4.0)
    edges = np.concatenate([start, start + np.cumsum(dts, 1, dtype=F64).astype(F32)], 1)
    ts, te = np.ascontiguousarray(edges[:, :-1]), np.ascontiguousarray(edges[:, 1:])
    sg = np.zeros((R, S), F32)
    for r, ws in enumerate(walls):
        for q in ws:
            sg[r, q] = F32(128.0) / dts[r, q]
    has_wall = np.array([len(ws) > 0 for ws in walls])
    p = dict(ts=ts, te=te, sg=sg, walls=walls, has_wall=has_wall,
             dW=_dy(rng, (R, S), 1.0, -3, 3), dT=_dy(rng, (R, S), 0.5, -2, 2), dA=_dy(rng, (R, S), 0.5, -2, 2),
             dC=_dy(rng, (R, S + 1), 0.25, -1, 1), dS=np.concatenate([_dy(rng, (R, 1), 0.5, -2, 2), _dy(rng, (R, 1), 0.25, -1, 1),
                                                                       np.full((R, 2), 7.0, F32)], 1),
             rgb=_dy(rng, (R, S, 3), 0.25, 0, 1), sky=rng.choice(np.array([0, 0.25, 0.5, 1.0], F32), size=(R, 3)),
             d_out=(rng.choice(np.array([0.5, 1.0, 2.0], F32), size=(R, 3)) * rng.choice(np.array([-1.0, 1.0], F32), size=(R, 3))),
             d_opa=_dy(rng, (R, 1), 0.5, -2, 2),
             # depth = sum(w mid) / 1e-6f on a ray without a wall: its gradient 1e6 d_dep mid rounds, so d_dep is 0 there
             d_dep=_dy(rng, (R, 1), 0.25, -1, 1) * has_wall[:, None].astype(F32))
    # preconditions, in fp32
    with np.errstate(under="ignore"):
        assert np.exp(F32(-128.0)) == F32(0) and np.exp(F32(-0.0)) == F32(1)
    _multiple(edges, 0.25, "edges")
    assert np.array_equal(te - ts, dts) and edges.dtype == F32
    sdt = sg * (te - ts)
    assert sdt.dtype == F32 and np.isin(sdt, (0.0, 128.0)).all()
    for r, ws in enumerate(walls):
        assert np.array_equal(np.flatnonzero(sdt[r]), np.array(sorted(ws), np.int64))
    # the scans: sigma dt (units of 128), cumsum of w (w is 0 or 1: at most one 1), the suffix scan (units of 2^-5:
    # g1 on 2^-2 times mid on 2^-3)
    mid = (ts.astype(F64) + te) / 2
    _multiple(mid, 0.125, "mid")
    _units(np.abs(sdt).sum(1), 128.0, "sigma dt")
    gw = np.abs(p["dW"]) + 4.0 + np.abs(p["dS"][:, 0:1]) + 14.0 + (np.abs(p["dS"][:, 1:2]) + np.abs(p["d_dep"])) * mid
    rf = ref_render(ts, te, sg)
    w01, T01 = rf["w"].astype(F32).astype(F64), rf["T"].astype(F32).astype(F64)
    assert np.isin(w01, (0, 1)).all() and np.isin(T01, (0, 1)).all() and (w01.sum(1) == has_wall).all()
    _units((gw * w01 + (np.abs(p["dT"]) + np.abs(p["dC"][:, :S])) * T01).sum(1), 2.0 ** -5, "suffix scan")
    _units((w01 * mid).sum(1), 0.125, "sum w mid")
    return p


def check_exact(got, want, what, residue=0.0, rounded=False):
    """Equal as numbers, entry by entry (no NaN; the sign of a zero is not held), to the fp64 reference, which must itself be
    an fp32 number.  Two stated exceptions: ``residue`` (wall probes: float64 keeps exp(-128) = 2.6e-56 where fp32 holds 0, so
    the reference may sit that far from the fp32 number) and ``rounded`` (rgb and d_rgb_sky of a wall probe: the kernel
    rounds the exact sky (1 - 1e-6f), sky a power of two, once)."""
    got, want = np.asarray(got), np.asarray(want, F64)
    assert got.dtype == F32 and got.shape == want.shape, f"{what}: dtype {got.dtype}, shape {got.shape} vs {want.shape}"
    w32 = want.astype(F32).astype(F64)
    if not rounded:
        off = np.abs(want - w32)
        assert (off <= residue).all(), (f"{what}: the fp64 reference is not an fp32 number at {int((off > residue).sum())} entries "
                                        f"(worst {off.max():.3e})")
    want = w32
    bad = ~(got.astype(F64) == want)
    if bad.any():
        i = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ from the fp64 reference; first at {i}: "
                             f"got {got[i]!r}, want {want[i]!r}")


def check_wall_render(p, got, what):
    """render_weights outputs (dict: weights, trans, alphas, cdfs, stats, t_mid, t_dist, d_sigma) on a wall probe."""
    rf, rb = ref_render_all(p)
    R, S = rf["x"].shape
    for r, ws in enumerate(p["walls"]):   # the stated values
        want = (1.0, rf["mid"][r, ws[0]], rf["mid"][r, ws[0]]) if ws else (0.0, 0.0, rf["mid"][r, S - 1])
        assert tuple(rf["stats"][r, :3]) == want, f"{what}: fp64 reference stats {rf['stats'][r]} vs {want}"
    assert (rf["cdfs"][:, S] == 1).all()
    for k in ("weights", "trans", "alphas", "cdfs", "stats", "t_mid", "t_dist"):
        if k in got:
            check_exact(got[k], rf[k], f"{what} {k}", residue=EXP128)
    if "d_sigma" in got:
        check_exact(got["d_sigma"], rb["d_sigma"], f"{what} d_sigma", residue=EXP128)


def check_wall_composite(p, got, what):
    """composite_rgb outputs and gradients on a wall probe; the clamp passes the gradient on a wall ray (sum w == 1, on the
    bound) and cuts it on a ray without one (sum w == 0 < 1e-6)."""
    rf, ep, rb = ref_composite_all(p)
    assert np.array_equal(ep["passes"], p["has_wall"]) and np.array_equal(rf["stats"][:, 0], p["has_wall"].astype(F64))
    want = dict(weights=rf["w"], trans=rf["T"], t_mid=rf["mid"], t_dist=rf["dts"], opacity=ep["opacity"], depth=ep["depth"],
                median=ep["median"], rgb_out=ep.get("rgb"), d_sigma=rb["d_sigma"], d_rgb=ep.get("d_rgb"), d_sky=ep.get("d_sky"))
    for k, v in want.items():
        if v is not None and got.get(k) is not None:
            check_exact(np.asarray(got[k]).reshape(v.shape), v, f"{what} {k}", residue=EXP128, rounded=k in ("rgb_out", "d_sky"))


def accumulate_probe(R, S, C, seed=0):
    rng = np.random.default_rng(seed + 7 * S + 131 * (C or 0) + R)
    p = dict(w=_dy(rng, (R, S), 1 / 16, 0, 1), v=None if C is None else _dy(rng, (R, S, C), 1 / 8, -2, 2),
             go=_dy(rng, (R, C or 1), 0.5, -2, 2))
    rf = ref_accumulate(p["w"], p["v"], p["go"])
    _units(rf["out_abs"], 2.0 ** -7, "accumulate forward")
    _units(rf["d_w_abs"] + 1, 2.0 ** -4, "accumulate d_w")
    return p


def check_accumulate(p, out, d_w, d_v, what):
    rf = ref_accumulate(p["w"], p["v"], p["go"])
    check_exact(out, rf["out"], f"{what} out")
    check_exact(d_w, rf["d_w"], f"{what} d_w")
    if p["v"] is not None:
        check_exact(d_v, rf["d_v"], f"{what} d_v")


def _blend_common(rng, R, S):
    sig = rng.choice(np.array([32.0, 64.0], F32), size=(R, S))
    assert (sig + EPS).dtype == F32 and np.array_equal(sig + EPS, sig), "sig + 1e-6f != sig in fp32"
    inv = F32(1) / (sig + EPS)
    assert np.array_equal(np.frexp(inv)[0], np.full(inv.shape, 0.5, F32)), "1 / sig is not a power of two"
    return dict(w=_dy(rng, (R, S), 1 / 8, 0, 1), sig=sig, ss=_dy(rng, (R, S), 0.25, 0, 8), sd=_dy(rng, (R, S), 0.25, 0, 8))


def blend_probe(R, S, with_shadow, seed=0):
    rng = np.random.default_rng(seed + 3 * S + R + 1000 * with_shadow)
    p = _blend_common(rng, R, S)
    p.update(rs=_dy(rng, (R, S, 3), 1 / 8, 0, 1), rd=_dy(rng, (R, S, 3), 1 / 8, 0, 1),
             sh=rng.choice(np.array([0, 0.25, 0.5, 1.0], F32), size=(R, S)) if with_shadow else None,
             g_rgb=_dy(rng, (R, 3), 0.5, -2, 2), g_sh=_dy(rng, (R, 1), 0.5, -2, 2) if with_shadow else None)
    rf = ref_blend(p, den=p["sig"] + EPS)
    # units: w 2^-3, a 2^-8, (1 - shadow) 2^-2, colours 2^-3 -> 2^-16 per term of the forward sum
    _units(rf["acc_abs"], 2.0 ** -16, "blend forward")
    for k in ("d_w", "d_sig", "d_sh"):
        if k in rf:
            assert np.array_equal(rf[k].astype(F32).astype(F64), rf[k]), f"blend {k} not representable"
    return p


def check_blend(p, got, what, wide=False):
    rf = (ref_blend_wide if wide else ref_blend)(p, den=p["sig"] + EPS)
    for k in (WIDE_KEYS if wide else BLEND_KEYS):
        if k in rf:
            check_exact(np.asarray(got[k]).reshape(rf[k].shape), rf[k], f"{what} {k}")


def blend_wide_probe(R, S, C, seed=0):
    rng = np.random.default_rng(seed + 3 * S + R + 17 * C)
    p = _blend_common(rng, R, S)
    p.update(fs=_dy(rng, (R, S, C), 0.25, -2, 2), fd=_dy(rng, (R, S, C), 0.25, -2, 2), g_acc=_dy(rng, (R, C), 0.5, -2, 2))
    if R * S > 100000:
        return p          # the cap case: C = 1, one product per sum -- nothing to budget
    rf = ref_blend_wide(p, den=p["sig"] + EPS)
    _units(rf["acc_abs"], 2.0 ** -13, "wide forward")       # w 2^-3, a 2^-8, features 2^-2
    _units(rf["d_w_abs"], 2.0 ** -11, "wide d_w")           # a 2^-8, g 2^-1, features 2^-2
    _units(rf["d_sig_abs"], 2.0 ** -20, "wide d_sig")       # w 2^-3, mS 2^-3, sigma_s 2^-2, inv^2 >= 2^-12
    return p


def epilogue_probe(k=3, seed=0):
    """6 k rays: sum w walks the six special values; everything else dyadic."""
    rng = np.random.default_rng(seed)
    R = 6 * k
    st = np.stack([np.tile(np.array(SPECIAL_WSUM, F32), k), _dy(rng, (R,), 0.25, 0, 8), _dy(rng, (R,), 0.125, 0, 50),
                   np.full(R, 7.0, F32)], 1)
    return dict(stats=st, acc=_dy(rng, (R, 3), 1 / 8, 0, 1), sky=rng.choice(np.array([0, 0.25, 0.5, 1.0], F32), size=(R, 3)),
                d_opa=_dy(rng, (R, 1), 0.5, 0.5, 2), d_dep=_dy(rng, (R, 1), 0.25, -1, 1),
                d_out=(rng.choice(np.array([0.5, 1.0, 2.0], F32), size=(R, 3)) * rng.choice(np.array([-1.0, 1.0], F32), size=(R, 3))))


# ---------------------------------------------------------------------------------------------------- realistic rays
def realistic(R, S, seed=None):
    """Sorted edges in [0.1, 50], sigma = rand^3 * 2, ray 0 all zero, ray 1 saturated; normal upstream gradients."""
    rng = np.random.default_rng(REAL_SEED + 100 * S + R if seed is None else seed)
    edges = np.sort(rng.random((R, S + 1)) * 49.9 + 0.1, 1).astype(F32)
    sg = (rng.random((R, S)) ** 3 * 2.0).astype(F32)
    sg[0] = 0.0
    sg[1] = 50.0
    def n(*sh):
        return rng.standard_normal(sh).astype(F32)
    return dict(ts=np.ascontiguousarray(edges[:, :-1]), te=np.ascontiguousarray(edges[:, 1:]), sg=sg, dW=n(R, S), dT=n(R, S), dA=n(R, S),
                dC=n(R, S + 1), dS=np.concatenate([n(R, 2), np.full((R, 2), 7.0, F32)], 1), rgb=rng.random((R, S, 3)).astype(F32),
                sky=rng.random((R, 3)).astype(F32), d_out=n(R, 3), d_opa=n(R, 1), d_dep=n(R, 1))


def realistic_blend(R, S, C=None, seed=5):
    rng = np.random.default_rng(seed + S + (C or 0))
    def f(*sh):
        return rng.random(sh).astype(F32)
    def n(*sh):
        return rng.standard_normal(sh).astype(F32)
    ss, sd = f(R, S) ** 3 * 5, f(R, S) ** 3 * 5
    ss[0, 0] = sd[0, 0] = 0.0      # empty sample: ratios 0 / 1e-6
    p = dict(w=f(R, S) / S, ss=ss, sd=sd, sig=ss + sd)
    if C is None:
        p.update(rs=f(R, S, 3), rd=f(R, S, 3), sh=f(R, S), g_rgb=n(R, 3), g_sh=n(R, 1))
    else:
        p.update(fs=n(R, S, C), fd=n(R, S, C), g_acc=n(R, C))
    return p


# --------------------------------------------------------------------------- checks shared by the CPU and the GPU tests
def _mid32(p):
    return (np.asarray(p["ts"], F32) + np.asarray(p["te"], F32)) / F32(2)


def check_real_render(p, got, what, report=None, allow_ambiguous=False):
    """render_weights on arbitrary inputs: every entry of every output and of d_sigma inside its bound, t_mid / t_dist the
    fp32 operations themselves, the median exact (a ray within the bound of 0.5 may slip by one sample when allowed)."""
    rf, g = ref_render_all(p)
    bd = B.render_bounds(rf)
    R, S = rf["x"].shape
    for k in ("weights", "trans", "alphas", "cdfs"):
        B.assert_err_bound(got[k], rf[k], bd[k], f"{what} {k}", report)
    st = np.asarray(got["stats"])
    B.assert_err_bound(st[:, 0], rf["stats"][:, 0], bd["wsum"], f"{what} sum w", report)
    B.assert_err_bound(st[:, 1], rf["stats"][:, 1], bd["wmid"], f"{what} sum w mid", report)
    assert (st[:, 3] == 0).all()
    check_median(p, rf, bd, st[:, 2], what, allow_ambiguous)
    for k, v in (("t_mid", _mid32(p)), ("t_dist", np.asarray(p["te"], F32) - np.asarray(p["ts"], F32))):
        if got.get(k) is not None:
            assert np.array_equal(np.asarray(got[k]), v), f"{what} {k}"
    if got.get("d_sigma") is not None:
        B.assert_err_bound(got["d_sigma"], g["d_sigma"], B.dsigma_bound(rf, bd, g), f"{what} d_sigma", report)
    return rf, bd


def check_median(p, rf, bd, med, what, allow_ambiguous=False):
    R, S = rf["x"].shape
    amb = B.median_ambiguous(rf, bd)
    assert allow_ambiguous or not amb.any(), f"{what}: rays {np.flatnonzero(amb)} have a cumsum of w within its bound of 0.5"
    mid = _mid32(p)
    idx = np.minimum((rf["cw"] < 0.5).sum(1), S - 1)
    med = np.asarray(med).reshape(R)
    for r in range(R):
        if amb[r]:
            assert med[r] in mid[r, max(idx[r] - 1, 0):idx[r] + 2], f"{what}: median of ambiguous ray {r}"
        else:
            assert med[r] == mid[r, idx[r]], f"{what}: median of ray {r}: {med[r]!r} vs sample {idx[r]}: {mid[r, idx[r]]!r}"


def check_real_composite(p, got, what, report=None, allow_ambiguous=False, wsum=None):
    """composite_rgb against the fp64 restatement directly (render -> accumulate -> epilogue and back), every ray to the same
    bounds.  ``wsum``: the kernels' own sum w (render_weights' stats[:, 0], bitwise the fused kernel's).  It tells which
    branch of the clamp's gradient the kernel took; the restatement is evaluated with that branch (``clamp_branch`` admits
    a difference from fp64's only within the bound of sum w), so a ray on a clamp bound is held like any other."""
    rf = ref_render(p["ts"], p["te"], p["sg"])
    bd = B.render_bounds(rf)
    took = None if wsum is None else clamp_branch(rf, bd["wsum"], wsum)
    rf, ep, g = ref_composite_all(p, took)
    R, S = rf["x"].shape
    a = np.abs
    e_acc = None
    if ep["acc"] is not None:
        e_acc = (bd["w"][..., None] * a(np.asarray(p["rgb"], F64))).sum(1) + B.c_accumulate(S, 3) * B.U * ep["acc_abs"]
    eb = B.epilogue_bounds(ep, bd["wsum"], bd["wmid"], e_acc)
    B.assert_err_bound(got["weights"], rf["w"], bd["w"], f"{what} weights", report)
    B.assert_err_bound(got["trans"], rf["T"], bd["T"], f"{what} trans", report)
    B.assert_err_bound(got["opacity"], ep["opacity"], eb["opacity"], f"{what} opacity", report)
    B.assert_err_bound(got["depth"], ep["depth"], eb["depth"], f"{what} depth", report)
    check_median(p, rf, bd, got["median"], what, allow_ambiguous)
    assert np.array_equal(np.asarray(got["t_mid"]), _mid32(p))
    if got.get("rgb_out") is not None:
        B.assert_err_bound(got["rgb_out"], ep["rgb"], eb["rgb"], f"{what} rgb", report)
    g.update(e_g0=eb["g0"], e_g1=eb["g1"])
    B.assert_err_bound(got["d_sigma"], g["d_sigma"], B.dsigma_bound(rf, bd, g), f"{what} d_sigma", report)
    if took is not None:
        x = rf["stats"][:, 0]
        other = took != ((x >= F64(EPS)) & (x <= 1.0))
        if other.any():
            ds, e_ds = np.asarray(got["d_sigma"]), B.dsigma_bound(rf, bd, g)
            B.assert_err_bound(ds[other], g["d_sigma"][other], e_ds[other],
                               f"{what} d_sigma, the {int(other.sum())} rays on the other clamp branch than fp64", report)
    if got.get("d_rgb") is not None:
        gg = a(np.asarray(p["d_out"], F64)).reshape(R, 1, 3)
        B.assert_err_bound(got["d_rgb"], ep["d_rgb"], bd["w"][..., None] * gg + B.U * a(ep["d_rgb"]), f"{what} d_rgb", report)
    if got.get("d_sky") is not None:
        B.assert_err_bound(got["d_sky"], ep["d_sky"], eb["d_sky"], f"{what} d_sky", report)
    return eb


def check_epilogue_probe(p, got, what):
    """ray_epilogue on ``epilogue_probe``: opacity, depth (one correctly rounded division), the median, g1 and d_sky are the
    fp64 values rounded once; rgb where sky (1 - o) is exact; the clamp's gradient mask exactly; the rest inside the bound."""
    ep = ref_epilogue(p["stats"], p["acc"], p["sky"], p["d_opa"], p["d_dep"], p["d_out"])
    eb = B.epilogue_bounds(ep)
    R = ep["opacity"].shape[0]
    def eq(g_, w_, k):
        return _same(np.asarray(g_).reshape(np.shape(w_)), np.asarray(w_, F64).astype(F32), f"{what} {k}")
    check_exact(np.asarray(got["opacity"]).reshape(R), ep["opacity"], f"{what} opacity")
    eq(got["depth"], ep["depth"], "depth")
    eq(got["median"], ep["median"], "median")
    rgb = np.asarray(got["rgb"])
    exact = ((ep["opacity"] == 1.0)[:, None] | (ep["sky"] == 0)) & np.ones((R, 3), bool)
    assert exact.any() and (~exact).any()
    assert np.array_equal(rgb[exact], ep["rgb"].astype(F32)[exact]), f"{what} rgb where sky (1 - o) is exact"
    B.assert_err_bound(rgb, ep["rgb"], eb["rgb"], f"{what} rgb")
    ds = np.asarray(got["d_stats"])
    on_bound = np.isin(p["stats"][:, 0], (EPS, F32(1)))
    assert (ep["go"][on_bound] != 0).any() and ep["passes"][on_bound].all() and (~ep["passes"]).sum() >= R // 2
    assert (ds[~ep["passes"], 0] == 0).all(), f"{what}: gradient passes outside the clamp range"
    assert ((ds[:, 0] != 0) == (ep["g0"] != 0)).all(), f"{what}: clamp gradient mask"
    B.assert_err_bound(ds[:, 0], ep["g0"], eb["g0"], f"{what} d sum w")
    eq(ds[:, 1], ep["g1"], "d sum w mid")
    assert (ds[:, 2:] == 0).all()
    assert np.array_equal(np.asarray(got["d_acc"]), p["d_out"]), f"{what} d_acc"
    eq(got["d_sky"], ep["d_sky"], "d_sky")


def _same(got, want, what):
    n_bad = int((got != want).sum())
    assert got.dtype == F32 and n_bad == 0, f"{what}: {n_bad} entries differ from the fp64 value rounded once"


def check_real_accumulate(p, out, d_w, d_v, what, report=None):
    rf = ref_accumulate(p["w"], p["v"], p["go"])
    S = np.shape(p["w"])[1]
    C = None if p["v"] is None else np.shape(p["v"])[2]
    B.assert_err_bound(out, rf["out"], B.c_accumulate(S, C) * B.U * rf["out_abs"], f"{what} out", report)
    B.assert_err_bound(d_w, rf["d_w"], (0.0 if C is None else B.c_accumulate_dw(C)) * B.U * rf["d_w_abs"], f"{what} d_w", report)
    if C is not None:
        B.assert_err_bound(d_v, rf["d_v"], B.U * rf["d_v_abs"], f"{what} d_v", report)


def check_real_blend(p, got, what, wide=False, report=None):
    rf = (ref_blend_wide if wide else ref_blend)(p)
    S = np.shape(p["w"])[1]
    c = B.blend_c(S, np.shape(p["fs"])[2] if wide else None)
    for k in (WIDE_KEYS if wide else BLEND_KEYS):
        if k in rf and got.get(k) is not None:
            B.assert_err_bound(got[k], rf[k], c[k] * B.U * rf[k + "_abs"], f"{what} {k}", report)


def check_real_blend_through_sum(p, got, what, wide=False, report=None):
    """As ``check_real_blend`` for a caller that formed sigma = sigma_s + sigma_d on the device (p["sig"]: that fp32 sum) and
    reads the gradients at the leaves: those of sigma_s and sigma_d hold d_sigma too, joined by one more fp32 addition."""
    rf = (ref_blend_wide if wide else ref_blend)(p)
    S = np.shape(p["w"])[1]
    c = B.blend_c(S, np.shape(p["fs"])[2] if wide else None)
    for k in (WIDE_KEYS if wide else BLEND_KEYS):
        if k in rf and got.get(k) is not None:
            ref, err = rf[k], c[k] * rf[k + "_abs"]
            if k in ("d_ss", "d_sd"):
                ref, err = ref + rf["d_sig"], err + c["d_sig"] * rf["d_sig_abs"] + rf[k + "_abs"] + rf["d_sig_abs"]
            B.assert_err_bound(got[k], ref, B.U * err, f"{what} {k}", report)
