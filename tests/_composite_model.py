"""numpy model of the compositing kernels' STRUCTURE (csrc/composite.hip and the ray epilogue of csrc/rayloss.hip), with
mutants.  Test helper, CPU only: tests/test_composite_bounds_cpu.py runs it against the probes of tests/_composite_probe.py.

It follows the kernels' operation order: 64-lane chunks with the carried prefix, chunk_base, the suffix scan with its carry,
tail-lane masking, the median's latch and last_lane, the small kernels' per-lane chains and wave sums, the wide forward's
four-wave split with its tail, the wide backward's quads.  A change to the summation structure of a kernel needs the same
change here.  ``mut`` selects one of ``MUTANTS``; ``dt`` the arithmetic (float32: the kernel; float64: the same function).
"""
import numpy as np

F32, F64 = np.float32, np.float64
W = 64                               # wavefront width
LANE = np.arange(W)
EPS = F32(1e-6)                      # the kernels' 1e-6f (clamp bound, blend denominator)

MUTANTS = {
    "carry2": "carry not added from chunk 2 on",
    "carry_prev": "carry taken from the previous chunk only",
    "incl": "inclusive sum used as exclusive",
    "suffix": "suffix carry dropped across chunks",
    "tail": "tail lanes unmasked (they read what lies behind the ray)",
    "latch": "median not latched at the first hit",
    "lane63": "last_mid from lane 63 instead of S-1-base",
    "dalpha": "d_alphas term dropped",
    "strict": "clamp gradient with strict inequalities",
    "acc_tail": "accumulate: last sample of a partial chunk dropped",
    "wide_tail": "wide forward: tail sample dropped",
    "quad_ray": "wide backward: a quad's ray index taken from its first sample",
}

# ------------------------------------------------------------------------------------------------- wave primitives
def wave_incl(v):
    """wave_inclusive_sum: Hillis-Steele over the last axis (64 lanes)."""
    off = 1
    while off < W:
        o = np.zeros_like(v)
        o[..., off:] = v[..., :-off]
        v = np.where(LANE >= off, v + o, v)
        off <<= 1
    return v


def wave_suffix(v):
    """wave_inclusive_suffix_sum: the same steps from the other end."""
    return wave_incl(v[..., ::-1])[..., ::-1]


def wave_sum(v):
    """wave_sum: xor butterfly; every lane holds the total."""
    off = W // 2
    while off:
        v = v + v[..., LANE ^ off]
        off >>= 1
    return v


def _lanes(flat, r, S, s, ok, unmask):
    """What the 64 lanes of every ray's wave load at samples ``s``: masked lanes hold 0.  Unmasked (mutant): they read the
    flat array behind the ray -- the next ray, wrapping at the end."""
    idx = r[:, None] * S + s[None, :]
    n = flat.shape[0]
    if unmask:
        return flat[idx % n]
    return np.where(ok[None, :], flat[np.minimum(idx, n - 1)], flat.dtype.type(0))


def _flat(x, dt, tail=()):
    return None if x is None else np.ascontiguousarray(x, dt).reshape((-1,) + tuple(tail))


# ------------------------------------------------------------------------------------------ model: scan kernels
def model_scan_fwd(ts, te, sg, rgb=None, mut="", dt=F32):
    """render_weights_fwd_kernel / the scan part of composite_rgb_fwd_kernel, all rays at once ([R, 64] per chunk)."""
    R, S = np.shape(sg)
    a_, b_, g_ = _flat(ts, dt), _flat(te, dt), _flat(sg, dt)
    c_ = _flat(rgb, dt, (3,))
    r = np.arange(R)
    def z(*sh):
        return np.zeros(sh, dt)
    out = dict(weights=z(R, S), trans=z(R, S), alphas=z(R, S), cdfs=z(R, S + 1), t_mid=z(R, S), t_dist=z(R, S))
    carry, prev, wcarry, median, last_mid = z(R), z(R), z(R), z(R), z(R)
    wsum, wmid, acc = z(R, W), z(R, W), z(R, W, 3)
    found = np.zeros(R, bool)
    un = mut == "tail"
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        for c, base in enumerate(range(0, S, W)):
            s = base + LANE
            ok = s < S
            okl = np.ones(W, bool) if un else ok
            a, b, g = (_lanes(x, r, S, s, ok, un) for x in (a_, b_, g_))
            sdt = g * (b - a)
            incl = wave_incl(sdt)
            cy = z(R) if (mut == "carry2" and c >= 2) else prev if mut == "carry_prev" else carry
            excl = cy[:, None] + (incl if mut == "incl" else incl - sdt)
            T = np.exp(-excl)
            al = dt(1) - np.exp(-sdt)
            w = np.where(okl, T * al, dt(0))
            mid = (a + b) / dt(2)
            k = int(ok.sum())
            sl = slice(base, base + k)
            out["weights"][:, sl], out["trans"][:, sl], out["alphas"][:, sl] = w[:, :k], T[:, :k], al[:, :k]
            out["cdfs"][:, sl], out["t_mid"][:, sl], out["t_dist"][:, sl] = (dt(1) - T)[:, :k], mid[:, :k], (b - a)[:, :k]
            if c_ is not None:
                for ch in range(3):
                    col = _lanes(c_[:, ch], r, S, s, ok, un)
                    acc[:, :, ch] = np.where(okl, acc[:, :, ch] + w * col, acc[:, :, ch])
            prev = incl[:, W - 1]
            carry = carry + prev
            cw = wcarry[:, None] + wave_incl(w)
            hit = okl & (cw >= dt(0.5))
            anyhit = hit.any(1)
            upd = anyhit & (~found | (mut == "latch"))
            median = np.where(upd, mid[r, hit.argmax(1)], median)
            found |= anyhit
            last_mid = mid[:, W - 1 if mut == "lane63" else min(S - 1 - base, W - 1)]
            wcarry = cw[:, W - 1]
            wsum, wmid = wsum + w, wmid + w * mid
        out["cdfs"][:, S] = 1
        out["stats"] = np.stack([wave_sum(wsum)[:, 0], wave_sum(wmid)[:, 0], np.where(found, median, last_mid), z(R)], 1)
        out["acc"] = np.stack([wave_sum(acc[:, :, ch])[:, 0] for ch in range(3)], 1) if c_ is not None else None
    return out


def model_scan_bwd(ts, te, sg, dW=None, dT=None, dA=None, g0=None, g1=None, rgb=None, g_rgb=None, weights=None, mut="", dt=F32):
    """render_weights_bwd_kernel (dW, dT, dA, g0 = d stats[:, 0], g1 = d stats[:, 1]) / the scan part of
    composite_rgb_bwd_kernel (rgb, g_rgb, weights: the accumulate backward folded in).  -> d_sigma[, d_rgb]"""
    R, S = np.shape(sg)
    a_, b_, g_ = _flat(ts, dt), _flat(te, dt), _flat(sg, dt)
    w_, T_, A_ = _flat(dW, dt), _flat(dT, dt), _flat(dA, dt)
    c_, sw_ = _flat(rgb, dt, (3,)), _flat(weights, dt)
    r = np.arange(R)
    def z(*sh):
        return np.zeros(sh, dt)
    g0 = z(R) if g0 is None else np.asarray(g0, dt).reshape(R)
    g1 = z(R) if g1 is None else np.asarray(g1, dt).reshape(R)
    gr = None if g_rgb is None else np.asarray(g_rgb, dt).reshape(R, 3)
    n_chunks = (S + W - 1) // W
    un = mut == "tail"
    ds = z(R, S)
    d_rgb = z(R, S, 3) if (c_ is not None and gr is not None) else None
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        chunk_base, carry = z(R, n_chunks), z(R)
        for c in range(n_chunks):
            s = c * W + LANE
            ok = s < S
            a, b, g = (_lanes(x, r, S, s, ok, un) for x in (a_, b_, g_))
            tot = wave_sum(g * (b - a))[:, 0]
            chunk_base[:, c] = z(R) if (mut == "carry2" and c >= 2) else carry
            carry = tot if mut == "carry_prev" else carry + tot
        suffix = z(R)
        for c in range(n_chunks - 1, -1, -1):
            s = c * W + LANE
            ok = s < S
            okl = np.ones(W, bool) if un else ok
            a, b, g = (_lanes(x, r, S, s, ok, un) for x in (a_, b_, g_))
            dts = b - a
            sdt = g * dts
            incl = wave_incl(sdt)
            excl = chunk_base[:, c, None] + (incl if mut == "incl" else incl - sdt)
            T, e = np.exp(-excl), np.exp(-sdt)
            w = T * (dt(1) - e)
            gw = z(R, W) if w_ is None else _lanes(w_, r, S, s, ok, un)
            k = int(ok.sum())
            if d_rgb is not None:
                acc = z(R, W)
                for ch in range(3):
                    acc = acc + gr[:, ch, None] * _lanes(c_[:, ch], r, S, s, ok, un)
                gw = np.where(okl, gw + acc, gw)
                ws = _lanes(sw_, r, S, s, ok, False)
                for ch in range(3):
                    d_rgb[:, c * W:c * W + k, ch] = (ws * gr[:, ch, None])[:, :k]
            gw = gw + (g0[:, None] + g1[:, None] * ((a + b) / dt(2)))
            gT = z(R, W) if T_ is None else _lanes(T_, r, S, s, ok, un)
            gA = z(R, W) if A_ is None else _lanes(A_, r, S, s, ok, un)
            term = np.where(okl, gw * w + gT * T, dt(0))
            sfx = wave_suffix(term)
            later = suffix[:, None] + (sfx - term)
            val = gw * T * e - later
            if mut != "dalpha":
                val = val + gA * e
            ds[:, c * W:c * W + k] = (dts * val)[:, :k]
            if mut != "suffix":
                suffix = suffix + sfx[:, 0]
    return (ds, d_rgb) if d_rgb is not None else ds


def model_epilogue_fwd(stats, acc=None, sky=None, dt=F32):
    """ray_epilogue_fwd_kernel / the lane-0 tail of composite_rgb_fwd_kernel -> opacity, depth, median, rgb."""
    st = np.asarray(stats, dt)
    o = np.minimum(np.maximum(st[:, 0], dt(EPS)), dt(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = st[:, 1] / o
    rgb = None
    if acc is not None:
        rgb = np.asarray(acc, dt)
        if sky is not None:
            rgb = rgb + np.asarray(sky, dt) * (dt(1) - o)[:, None]
    return o, depth, st[:, 2], rgb


def model_epilogue_bwd(stats, sky=None, do=None, dd=None, drgb=None, mut="", dt=F32):
    """ray_epilogue_bwd_kernel / the per-ray head of composite_rgb_bwd_kernel -> g0, g1, d_sky."""
    st = np.asarray(stats, dt)
    R = st.shape[0]
    o = np.minimum(np.maximum(st[:, 0], dt(EPS)), dt(1))
    go = np.zeros(R, dt) if do is None else np.asarray(do, dt).reshape(R).copy()
    gd = np.zeros(R, dt) if dd is None else np.asarray(dd, dt).reshape(R)
    go = go - gd * st[:, 1] / (o * o)
    dsky = None
    if drgb is not None and sky is not None:
        g, k = np.asarray(drgb, dt).reshape(R, 3), np.asarray(sky, dt).reshape(R, 3)
        for ch in range(3):
            go = go - g[:, ch] * k[:, ch]
        dsky = g * (dt(1) - o)[:, None]
    x = st[:, 0]
    mask = ((x > dt(EPS)) & (x < dt(1))) if mut == "strict" else ((x >= dt(EPS)) & (x <= dt(1)))
    return np.where(mask, go, dt(0)), gd / o, dsky


def model_composite(p, mut="", dt=F32):
    """composite_rgb forward and backward on a probe / input dict ``p`` (keys of ``wall_probe``)."""
    f = model_scan_fwd(p["ts"], p["te"], p["sg"], p.get("rgb"), mut, dt)
    o, depth, med, out = model_epilogue_fwd(f["stats"], f["acc"], p.get("sky") if f["acc"] is not None else None, dt)
    g0, g1, dsky = model_epilogue_bwd(f["stats"], p.get("sky"), p.get("d_opa"), p.get("d_dep"), p.get("d_out"), mut, dt)
    res = model_scan_bwd(p["ts"], p["te"], p["sg"], p.get("dW"), p.get("dT"), None, g0, g1, p.get("rgb"), p.get("d_out"),
                         f["weights"], mut, dt)
    ds, d_rgb = res if isinstance(res, tuple) else (res, None)
    return dict(weights=f["weights"], trans=f["trans"], t_mid=f["t_mid"], t_dist=f["t_dist"], opacity=o, depth=depth, median=med,
                rgb_out=out, d_sigma=ds, d_rgb=d_rgb, d_sky=dsky)


def model_render(p, mut="", dt=F32):
    """render_weights forward and backward on ``p``; the cdfs' gradient reaches trans as the wrapper forms it (-dC[:, :S])."""
    S = np.shape(p["sg"])[1]
    f = model_scan_fwd(p["ts"], p["te"], p["sg"], None, mut, dt)
    gT = np.asarray(p["dT"], dt) + (-np.asarray(p["dC"], dt)[:, :S])
    f["d_sigma"] = model_scan_bwd(p["ts"], p["te"], p["sg"], p["dW"], gT, p["dA"], p["dS"][:, 0], p["dS"][:, 1], mut=mut, dt=dt)
    return f


# ------------------------------------------------------------------------------ model: accumulate and the two blends
def _lane_chain(x, dt, drop_tail=False):
    """[R, S, ...] -> [R, 64, ...]: lane l adds its samples l, l + 64, ... in order (the small kernels' per-lane loop)."""
    R, S = x.shape[:2]
    if drop_tail and S % W:
        x = x[:, :S - 1]
        S -= 1
    n = (S + W - 1) // W
    pad = np.zeros((R, n * W) + x.shape[2:], dt)
    pad[:, :S] = x
    pad = pad.reshape((R, n, W) + x.shape[2:])
    acc = np.zeros((R, W) + x.shape[2:], dt)
    for c in range(n):
        acc = acc + pad[:, c]
    return acc


def _wsum_lanes(acc):
    """wave_sum over axis 1 of [R, 64, ...] -> [R, ...]."""
    return np.moveaxis(wave_sum(np.moveaxis(acc, 1, -1)), -1, 1)[:, 0]


def model_accumulate(w, v, go, mut="", dt=F32):
    """accumulate_fwd/bwd (small: C <= 8 or values None; wide otherwise) -> out, d_w, d_v."""
    w, go = np.asarray(w, dt), np.asarray(go, dt)
    R, S = w.shape
    if v is None:
        out = _wsum_lanes(_lane_chain(w, dt, mut == "acc_tail"))[:, None]
        return out, np.broadcast_to(go, (R, S)).astype(dt), None
    v = np.asarray(v, dt)
    C = v.shape[2]
    if C <= 8:
        out = _wsum_lanes(_lane_chain(w[:, :, None] * v, dt, mut == "acc_tail"))
        d_w = np.zeros((R, S), dt)
        for c in range(C):
            d_w = d_w + go[:, None, c] * v[:, :, c]
    else:
        out = np.zeros((R, C), dt)
        for s in range(S):
            out = out + w[:, s, None] * v[:, s]
        prod = np.moveaxis(go[:, None, :] * v, 2, 1)                 # [R, C, S]: lanes walk the channels
        d_w = _wsum_lanes(_lane_chain(prod, dt))
    return out, d_w, w[:, :, None] * go[:, None, :]


def model_blend(p, dt=F32):
    """blend_accumulate_fwd/bwd on a ``blend_probe`` dict -> dict of outputs and gradients."""
    def g(k):
        return None if p.get(k) is None else np.asarray(p[k], dt)
    w, sig, ss, sd, rs, rd, sh, g_rgb, g_sh = (g(k) for k in ("w", "sig", "ss", "sd", "rs", "rd", "sh", "g_rgb", "g_sh"))
    inv = dt(1) / (sig + dt(EPS))
    a, b = ss * inv, sd * inv
    s_ = np.zeros_like(w) if sh is None else sh
    ka = a * (dt(1) - s_)
    mix = ka[..., None] * rs + b[..., None] * rd
    out = dict(acc=_wsum_lanes(_lane_chain(w[..., None] * mix, dt)))
    gs = np.zeros(w.shape[0], dt) if (sh is None or g_sh is None) else g_sh.reshape(-1)
    if sh is not None:
        out["acs"] = _wsum_lanes(_lane_chain(w * s_ * s_, dt))
    G = g_rgb[:, None, :]
    gS = G[..., 0] * rs[..., 0] + G[..., 1] * rs[..., 1] + G[..., 2] * rs[..., 2]
    gD = G[..., 0] * rd[..., 0] + G[..., 1] * rd[..., 1] + G[..., 2] * rd[..., 2]
    out["d_w"] = ka * gS + b * gD + gs[:, None] * s_ * s_
    out["d_rs"], out["d_rd"] = G * (w * ka)[..., None], G * (w * b)[..., None]
    if sh is not None:
        out["d_sh"] = w * (dt(2) * gs[:, None] * s_ - a * gS)
    da, db = w * (dt(1) - s_) * gS, w * gD
    out["d_ss"], out["d_sd"], out["d_sig"] = da * inv, db * inv, -(da * ss + db * sd) * inv * inv
    return out


def model_blend_wide(p, mut="", dt=F32):
    """blend_accumulate_wide_fwd (four waves per ray: wave k takes samples k, k + 4, ... two at a time, then the tail) and
    _bwd (a wave takes four consecutive samples of the flat (ray, sample) range; lanes walk the channels)."""
    def g(k):
        return np.asarray(p[k], dt)
    w, sig, ss, sd, fs, fd, up = (g(k) for k in ("w", "sig", "ss", "sd", "fs", "fd", "g_acc"))
    R, S, C = fs.shape
    inv = dt(1) / (sig + dt(EPS))
    wa, wb = ss * inv, sd * inv
    def term(s):
        return w[:, s, None] * (wa[:, s, None] * fs[:, s] + wb[:, s, None] * fd[:, s])
    part = []
    for k in range(4):
        a0, a1, s = np.zeros((R, C), dt), np.zeros((R, C), dt), k
        while s + 4 < S:
            a0, a1 = a0 + term(s), a1 + term(s + 4)
            s += 8
        if s < S and mut != "wide_tail":
            a0 = a0 + term(s)
        part.append(a0 + a1)
    out = dict(acc=(part[0] + part[1]) + (part[2] + part[3]))
    n = R * S
    i = np.arange(n)
    rr = ((i // 4) * 4 // S) if mut == "quad_ray" else i // S
    fw, fss, fsd, finv = (x.reshape(n) for x in (w, ss, sd, inv))
    G = up[rr]                                                        # [n, C]
    def pad(x):   # [n, C] -> [n]
        return _wsum_lanes(_lane_chain(np.moveaxis(x[None], 2, 1), dt))[0]
    mS, mD = pad(G * fs.reshape(n, C)), pad(G * fd.reshape(n, C))
    out["d_fs"] = (G * (fw * fss * finv)[:, None]).reshape(R, S, C)
    out["d_fd"] = (G * (fw * fsd * finv)[:, None]).reshape(R, S, C)
    a_, b_ = fss * finv, fsd * finv
    out["d_w"] = (a_ * mS + b_ * mD).reshape(R, S)
    da, db = fw * mS, fw * mD
    out["d_ss"], out["d_sd"] = (da * finv).reshape(R, S), (db * finv).reshape(R, S)
    out["d_sig"] = (-(da * fss + db * fsd) * finv * finv).reshape(R, S)
    return out
