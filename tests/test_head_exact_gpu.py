"""Exact-arithmetic probes of the MLP head kernels (tests/_head_probe.py has the argument and the builders).

Inputs on a fixed-point grid with every partial sum inside 2^24 units: a correct kernel -- fp32 MFMA, bf16x3 MFMA, any
tile order, any atomics -- returns bitwise the fp64 result.  One layer of a stack is probed at a time; the other layers
copy values exactly (signed permutations, +-x split over two ReLU units).  Three probes per layer put the value on the
plane pairs w_l x_h ("lh"), w_h x_l ("hl") and w_m x_m ("mm") of the six kept partial products.  Backward: pass "A"
feeds output gradients shaped like the probe's activations (the data-gradient GEMMs are probes of the same plane pairs),
pass "B" output gradients shaped like its weights on six rows only (rows 0, 15, 16, a middle row in another workgroup
and the two last rows of the ragged tail), which keeps the row reductions of the weight gradients exact.  An entry whose
own sum leaves the budget, or that is fed by such an entry, is not compared (``mlp_ref_bwd``); the covers printed are
the exact fractions.  Nonlinear outputs (trunc_exp density, sigmoid colours) are held to a few ulp of the activation of
the exact pre-activation.  Also: the trunc_exp side gradient around and above its clamp at every site, and the class
default 768-wide feature heads.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _head_probe as P
from tests._bounds import C_EXP, C_SIG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E15 = float(np.float32(np.exp(15.0)))   # the clamp constant as the kernels hold it
K_EXP, K_SIG = C_EXP, C_SIG              # ulp budgets of the activations (tests/_bounds.py)


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)
    return t.requires_grad_(True) if grad else t


def _n(t):
    return t.detach().float().cpu().numpy()


def _sparse_rows_only(g, n_rows):
    """Keep rows 0, 15, 16, a middle row, n-2, n-1 of g (at most six non-zero rows)."""
    keep = sorted({0, 15, 16, n_rows // 2 + 3, n_rows - 2, n_rows - 1} & set(range(n_rows)))
    out = np.zeros_like(g)
    out[keep] = g[keep]
    return out


def _thin(x, k):
    """x with only the first k non-zeros of each row kept."""
    x = x.copy()
    x[np.cumsum(x != 0, 1) > k] = 0.0
    return x


def _check_grads(tag, got: dict, want: dict, must_cover=()):
    cover = {}
    for name, t in got.items():
        if t is None or name not in want:
            continue
        ref, ok = want[name]
        c = P.assert_exact(f"{tag} {name}", _n(t), ref, np.where(ok, 0.0, np.inf), min_cover=1.0 if name in must_cover else 0.0)
        cover[name] = round(c, 3)
    print(f"\n[exact] {tag}: cover {cover}")


def _seeds(kind, rows, cols, seed):
    """Output gradients of passes A and B (module docstring)."""
    ga = P.operand_like(kind, rows, cols, seed, "b")
    gb = _sparse_rows_only(P.operand_like(kind, rows, cols, seed + 1, "a"), rows)
    return {"A": ga, "B": gb}


def _stack(kind, layer, widths, rows, seed, relu_last=False):
    """Weights, biases and input of a Linear stack with layer ``layer`` probed and the others copying."""
    n = len(widths) - 1
    Ws, Bs = [], []
    if layer == 0:
        w, x, b, _, _ = P.probe(kind, widths[1], widths[0], rows, seed)
    else:
        x = P.operand_like(kind, rows, widths[0], seed, "b")
    for i in range(n):
        if i == layer:
            if i > 0:
                w = P.operand_like(kind, widths[i + 1], widths[i], seed + 7, "a")
                b = P.grid_values(np.random.default_rng(seed + 9), (widths[i + 1],), 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)
            Ws.append(w); Bs.append(b)
        elif i < layer:
            Ws.append(P.positive_copy(widths[i + 1], widths[i])); Bs.append(np.zeros(widths[i + 1], np.float32))
        else:
            last = i == n - 1 and not relu_last
            Ws.append(P.signed_perm(widths[i + 1], widths[i], seed + 11 + i) if last else np.abs(P.signed_perm(widths[i + 1], widths[i], seed + 11 + i)))
            Bs.append(np.zeros(widths[i + 1], np.float32))
    return x, Ws, Bs


# ------------------------------------------------------------------------------------------ ops.linear (fp32 MFMA)
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("n_out,k,rows,act", [(64, 64, 1000, "relu"), (256, 64, 777, "relu"), (768, 256, 300, None), (3, 64, 129, None),
                                              (16, 40, 333, "relu")])
def test_linear_exact(hip_lib, kind, n_out, k, rows, act):
    """emer_linear_fwd / emer_linear_bwd (fp32-input MFMA, linear_dw + linear_dw_reduce): forward, dx, dW, db."""
    from emernerf_amd import ops
    w, x, b, _, _ = P.probe(kind, n_out, k, rows, seed=n_out + k)
    hs, pres = P.mlp_ref(x, [w], [b], [act == "relu"])
    for pas, g in _seeds(kind, rows, n_out, seed=rows).items():
        X, W, B = _t(x, True), _t(w, True), _t(b, True)
        y = ops.linear(X, W, B, act)
        P.assert_exact(f"linear {kind} fwd", _n(y), hs[-1])
        y.backward(_t(g))
        want = P.mlp_ref_bwd(hs, pres, [w], [act == "relu"], g)
        _check_grads(f"linear {kind} {n_out}x{k} pass {pas}", {"dx": X.grad, "dW0": W.grad, "db0": B.grad}, want,
                     must_cover=("dx",) if pas == "A" else ("dW0", "db0"))


# ------------------------------------------------------------------------------------------ neck / base MLP
@pytest.mark.parametrize("fusedw", [True, False])
@pytest.mark.parametrize("L,Fe,NG,N", [(16, 2, 64, 1000), (10, 4, 128, 777), (8, 1, 64, 33), (16, 2, 128, 20000)])
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("kind", P.KINDS)
def test_neck_exact(hip_lib, monkeypatch, kind, layer, L, Fe, NG, N, fusedw):
    """emer_neck_fwd, emer_neck_bwd + emer_wgrad_segmented (fusedw False) and emer_neck_bwd_fused (weight gradients in the
    kernel, neck_bwdw): geometry / semantic features exact, density within K_EXP u of exp(f0 - 1), every gradient exact."""
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_WGRAD", fusedw)
    K0 = L * Fe
    x, Ws, Bs = _stack(kind, layer, (K0, 64, NG), N, seed=K0 + NG + layer)
    hs, pres = P.mlp_ref(x, Ws, Bs, [True, False])
    enc_lm = np.ascontiguousarray(x.reshape(N, L, Fe).transpose(1, 0, 2))
    for pas, g in _seeds(kind, N, NG, seed=N + layer).items():
        t = [_t(enc_lm, True)] + [_t(v, True) for v in (Ws[0], Bs[0], Ws[1], Bs[1])]
        geo, sem, dens = fused.neck(*t)
        f = np.concatenate([_n(geo)] + ([_n(sem)] if sem is not None else []), 1)
        P.assert_exact(f"neck {kind} L{layer} fwd", f, hs[-1])
        P.assert_ulp(f"neck {kind} L{layer} density", _n(dens), _trunc_ref(hs[-1][:, 0], 0.0)[0], K_EXP)
        loss = (geo * _t(g[:, :64])).sum() + ((sem * _t(g[:, 64:])).sum() if sem is not None else 0.0)
        loss.backward()
        want = P.mlp_ref_bwd(hs, pres, Ws, [True, False], g)
        denc = _n(t[0].grad).transpose(1, 0, 2).reshape(N, K0)
        _check_grads(f"neck {kind} layer {layer} L{L}F{Fe}NG{NG}N{N} fusedw={fusedw} pass {pas}",
                     {"dx": torch.from_numpy(denc), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad}, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}"))


# ------------------------------------------------------------------------------------------ proposal density MLP
@pytest.mark.parametrize("fusedw", [True, False])
@pytest.mark.parametrize("L,Fe,N", [(8, 1, 1000), (4, 4, 333), (8, 1, 70000)])
@pytest.mark.parametrize("kind", P.KINDS)
def test_density_mlp_exact(hip_lib, monkeypatch, kind, L, Fe, N, fusedw):
    """density_fwd_kernel, emer_density_bwd_fused (fusedw) / emer_neck_bwd + streamed weight gradients (n_out = 1).

    Layer 0 is the probe; unit j gets a sparse +-1 weight row and is read back by layer 1 as f0 = 32 h_j + 16, so rows with
    h_j > 0 lie above the trunc_exp clamp (f0 - 1 > 15, the density overflows to inf on some) and their side gradient is
    gd fp32(e^15) exactly (gd a power of two): a 24-bit value whose m and l planes are occupied.  Exact by construction:
    * d enc on every row: one product side x 32 x W0[j, k] (+-1 or 0) per entry -- the w_h x_l / w_h x_m pairs of the
      data-gradient GEMM (all gd rows live);
    * db0, db1 and, for "lh" (X entries +-1), dW0: passes with gd non-zero on ONE row (first, middle and last clamped row:
      other tiles, workgroups and the ragged tail), where each of these entries is a single product.
    Every other gradient entry of these passes is held by the per-entry bounds of tests/test_fused_gpu.py::test_density_mlp."""
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_WGRAD", fusedw)
    K0 = L * Fe
    w0, x, b0, _, _ = P.probe(kind, 64, K0, N, seed=K0 + N)
    j = 5
    w0[j] = 0.0
    w0[j, [0, 1 % K0]] = [1.0, -1.0] if K0 > 1 else [1.0]
    b0[j] = 0.5
    w1 = np.zeros((1, 64), np.float32); w1[0, j] = 32.0
    b1 = np.array([16.0], np.float32)
    hs, pres = P.mlp_ref(x, [w0, w1], [b0, b1], [True, False])
    f0 = hs[-1][:, 0]
    clamped = f0 - 1.0 > 15.0
    assert 0.2 < clamped.mean() < 1.0, "probe broken: clamped fraction"
    assert (hs[1][:, j] > 0).sum() == clamped.sum()
    rows = np.flatnonzero(clamped & (x != 0).any(1))   # single-row passes: rows with a live side gradient and a non-empty input
    gd_all = np.where(np.arange(N) % 3 == 0, -0.5, 0.5).astype(np.float32)   # one magnitude: one grid for every row
    passes = {"all rows": gd_all}
    for r in (rows[0], rows[len(rows) // 2], rows[-1]):
        passes[f"row {r}"] = np.where(np.arange(N) == r, gd_all, 0.0).astype(np.float32)
    xin = np.ascontiguousarray(x.reshape(N, L, Fe).transpose(1, 0, 2))
    for name, gd in passes.items():
        t = [_t(xin, True)] + [_t(v, True) for v in (w0, b0, w1, b1)]
        dens = fused.density_mlp(*t)
        P.assert_ulp(f"density {kind}", _n(dens), _trunc_ref(f0, 0.0)[0], K_EXP)
        (dens * _t(gd)).sum().backward()
        side = gd * np.where(clamped, E15, np.exp(np.minimum(f0 - 1.0, 15.0)))
        want = P.mlp_ref_bwd(hs, pres, [w0, w1], [True, False], side[:, None], row_ok=clamped | (gd == 0))
        must = () if name == "all rows" else ("db0", "db1") + (("dW0",) if kind == "lh" else ())
        denc = _n(t[0].grad).transpose(1, 0, 2).reshape(N, K0)
        if name == "all rows":   # d enc[m, k] = (32 side_m) W0[j, k] on the clamped rows, 0 elsewhere: one product, every entry
            P.assert_exact(f"density {kind} L{L}F{Fe}N{N} fusedw={fusedw} d enc", denc,
                           (32.0 * side * clamped)[:, None] * w0[j].astype(np.float64)[None, :])
        got = {"dx": torch.from_numpy(denc), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad}
        _check_grads(f"density {kind} L{L}F{Fe}N{N} fusedw={fusedw} gd on {name}", got, want, must_cover=must)
        # the designed entries are non-zero: the probe compares real gradients, not structural zeros
        for m in must:
            assert np.count_nonzero(want[m][0]) >= 1, f"probe broken: {m} has no non-zero entry"
        if name == "all rows":
            assert np.count_nonzero(denc) >= clamped.sum(), "probe broken: d enc has too few non-zero entries"


# ------------------------------------------------------------------------------------------ register-resident plain heads
@pytest.fixture(params=[True, False], ids=["fusedw", "streamedw"])
def rmlp_mode(request, monkeypatch):
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_RMLP_WGRAD", request.param)
    return request.param


_RMLP = [((64, 64, 64, 64), 4096, None), ((64, 64, 3), 1000, None), ((40, 64, 64, 6), 777, (10, 4)), ((64, 64, 16), 3001, None)]


@pytest.mark.parametrize("widths,N,lm,layer", [(w, n, lm, i) for w, n, lm in _RMLP for i in range(len(w) - 1)])
@pytest.mark.parametrize("kind", P.KINDS)
def test_rmlp_exact(hip_lib, rmlp_mode, kind, layer, widths, N, lm):
    """emer_rmlp_fwd / emer_rmlp_bwd / emer_rmlp_bwd_fused (rmlp_bwdw), row-major (fused.seq_mlp) and level-major
    (fused.seq_mlp_lm): output and every gradient exact."""
    from emernerf_amd import fused, _lib
    n = len(widths) - 1
    x, Ws, Bs = _stack(kind, layer, widths, N, seed=sum(widths) + layer)
    relus = [True] * (n - 1) + [False]
    hs, pres = P.mlp_ref(x, Ws, Bs, relus)
    assert fused.rmlp_supported([torch.empty(w.shape) for w in Ws], widths[0], lm[1] if lm else 0)
    for pas, g in _seeds(kind, N, widths[-1], seed=N + layer).items():
        xin = np.ascontiguousarray(x.reshape(N, lm[0], lm[1]).transpose(1, 0, 2)) if lm else x
        X = _t(xin, True)
        Wt, Bt = [_t(w, True) for w in Ws], [_t(b, True) for b in Bs]
        out = (fused.seq_mlp_lm(X, Wt, Bt) if lm else fused.seq_mlp(X, Wt, Bt, _lib.ACT_NONE))
        P.assert_exact(f"rmlp {kind} L{layer} fwd", _n(out), hs[-1])
        out.backward(_t(g))
        want = P.mlp_ref_bwd(hs, pres, Ws, relus, g)
        dx = _n(X.grad).transpose(1, 0, 2).reshape(N, widths[0]) if lm else _n(X.grad)
        got = {"dx": torch.from_numpy(dx)}
        for i in range(n):
            got[f"dW{i}"], got[f"db{i}"] = Wt[i].grad, Bt[i].grad
        _check_grads(f"rmlp {kind} layer {layer} {widths} lm={bool(lm)} fusedw={rmlp_mode} pass {pas}", got, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}"))


# ------------------------------------------------------------------------------------------ rgb head (forward)
@pytest.mark.parametrize("R,S,Kh", [(16, 64, 49), (1031, 32, 49), (5, 16, 17)])
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("kind", P.KINDS)
def test_rgb_head_forward_exact(hip_lib, kind, layer, R, S, Kh):
    """emer_ray_pre_fwd + emer_rgb_head_fwd: the stored hidden activations a1, a2 exact (layer 0 over [hray | geo], layer 1
    over the skip concatenation [a1 | hray | geo]), the colours within K_SIG u of sigmoid of the exact pre-activation.
    The backward below the sigmoid has no exact input (the sigmoid derivative is not on a grid): it is held by the
    per-entry bounds of tests/test_fused_gpu.py::test_rgb_head (every FUSED_RGB_WGRAD / RGB_RECOMPUTE mode)."""
    from emernerf_amd import fused
    N, H, NG = R * S, 64, 64
    K0 = Kh + NG
    rng = np.random.default_rng(R + S + layer)
    # the probe's activation distribution over the per-ray part and geo alike
    xr = P.operand_like(kind, R, Kh, R + 1, "b")
    xg = P.operand_like(kind, N, NG, R + 2, "b")
    if layer == 1 and kind != "hl":   # at most 3 + 3 non-zeros per row: a1 (<= 6) and the skip inputs share one budget
        xr, xg = _thin(xr, 3), _thin(xg, 3)
    inp = np.concatenate([np.repeat(xr, S, 0), xg], 1)
    if layer == 0:
        w0 = P.operand_like(kind, H, K0, 3, "a")
        b0 = P.grid_values(rng, (H,), 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)
        w1 = np.concatenate([np.abs(P.signed_perm(H, H, 4)), np.zeros((H, K0), np.float32)], 1)   # a2 = a1
        b1 = np.zeros(H, np.float32)
    else:
        # layer 0 copies 32 of the inputs with both signs, layer 1 is the probe over [a1 | inp] (the skip concatenation)
        w0 = P.positive_copy(H, 32) @ np.eye(32, K0, dtype=np.float32)
        b0 = np.zeros(H, np.float32)
        wa = P.operand_like(kind, H, H, 5, "a")
        wi = P.operand_like(kind, H, K0, 6, "a")
        w1 = np.concatenate([wa, wi], 1).astype(np.float32)
        b1 = P.grid_values(rng, (H,), 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)
    w2 = np.zeros((3, H), np.float32)
    w2[np.arange(3), [1, 17, 40]] = [1.0, -0.5, 0.25]
    b2 = np.array([0.0, 0.5, -0.25], np.float32)
    hs0, _ = P.mlp_ref(inp, [w0], [b0], [True])
    a1 = hs0[1]
    hs1, _ = P.mlp_ref(np.concatenate([a1, inp], 1), [w1], [b1], [True])
    a2 = hs1[1]
    z = a2 @ w2.T.astype(np.float64) + b2
    saved = []
    ws = [_t(v, True) for v in (w0, b0, w1, b1, w2, b2)]
    with torch.autograd.graph.saved_tensors_hooks(lambda x: saved.append(x) or x, lambda x: x):
        rgb = fused.rgb_head(_t(xr, True), _t(xg, True), S, *ws)
    # saved (fused.py _RgbHeadFn): hray, geo, W0, W1, W2, a1, a2, out, ... (a1 / a2 absent when recomputed)
    acts = [x for x in saved if x.dim() == 2 and tuple(x.shape) == (N, H)][1:]   # [0] is geo
    if fused.rgb_recompute(R, S) == 0:
        assert len(acts) == 2, [tuple(x.shape) for x in saved]
        P.assert_exact(f"rgb {kind} L{layer} a1", _n(acts[0]), a1)
        P.assert_exact(f"rgb {kind} L{layer} a2", _n(acts[1]), a2)
    P.assert_ulp(f"rgb {kind} L{layer} colour", _n(rgb), 1.0 / (1.0 + np.exp(-z)), K_SIG)


# ------------------------------------------------------------------------------------------ trunc_exp above its clamp
def _clamp_values():
    """Pre-activations x (density = exp(x - 1)): below 15 + 1, at 16 - 1 ulp / 16 / 16 + 1 ulp, between 16 and 88, and
    above 89.7 where the density overflows to inf and its gradient must stay finite."""
    v = [-3.0, 0.5, 1.0, 9.75, 15.0, np.nextafter(np.float32(16.0), np.float32(0)), 16.0, np.nextafter(np.float32(16.0), np.float32(99)),
         17.0, 40.5, 88.0, 89.5, 89.75, 95.0, 120.0]
    return np.array(v, np.float32)


def _trunc_ref(x, gd):
    """(density, d density / d x) in fp64: exp(x - 1) of the fp32 x - 1 (inf past fp32), gd exp(min(x - 1, 15)) with the
    clamp at the fp32 value of e^15 (what the kernels compare against)."""
    xm1 = (x.astype(np.float32) - np.float32(1.0)).astype(np.float64)
    with np.errstate(over="ignore"):
        dens = np.exp(xm1)
    dens = np.where(dens > np.finfo(np.float32).max, np.inf, dens)
    side = gd * np.minimum(np.exp(np.minimum(xm1, 15.0)), E15)
    return dens, side


def _assert_side(name, got, want):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite gradient"
    P.assert_ulp(name, got, want, K_EXP)


def _assert_row_sum(name, got, terms):
    """got[j] = sum over rows of terms[:, j] (side gradients with their own C_EXP + 1 u each), within the per-addition bound
    of tests/_bounds.py: (c_head_bf16x3(rows) + C_EXP + 1) u sum |terms|."""
    from tests._bounds import C_EXP, c_head_bf16x3
    terms = np.asarray(terms, np.float64)
    ref, a = terms.sum(0), np.abs(terms).sum(0)
    err = np.abs(np.asarray(got, np.float64) - ref)
    lim = (c_head_bf16x3(terms.shape[0]) + C_EXP + 1) * P.U * a
    assert np.isfinite(got).all() and (err <= lim).all(), f"{name}: got {got}, fp64 {ref}, err / bound {err / np.maximum(lim, 1e-300)}"


def test_trunc_exp_clamp_elementwise(hip_lib):
    """ops.trunc_exp_column (emer_trunc_exp_fwd/bwd) and ops.aggregate3_density (emer_aggregate3_density_fwd/bwd)."""
    from emernerf_amd import ops
    x = _clamp_values()
    n = x.size
    gd = np.where(np.arange(n) % 2 == 0, 1.0, -0.25).astype(np.float32)
    dens_ref, side_ref = _trunc_ref(x, gd)
    feats = np.zeros((n, 4), np.float32); feats[:, 0] = x; feats[:, 1:] = 7.0
    F = _t(feats, True)
    d = ops.trunc_exp_column(F, 0)
    P.assert_ulp("trunc_exp_column fwd", _n(d), dens_ref, K_EXP)
    d.backward(_t(gd))
    _assert_side("trunc_exp_column bwd", _n(F.grad)[:, 0], side_ref)
    assert not _n(F.grad)[:, 1:].any()
    # aggregate3_density: density of the aggregated column 0 = (cur + 0.5 fwd + 0.5 bwd) / 2 -> choose cur = fwd = bwd = x / 1
    x3 = np.concatenate([feats, feats, feats], 0)
    X3 = _t(x3, True)
    agg, dens = ops.aggregate3_density(X3)
    xa = _n(agg)[:, 0]
    dens_ref3, side_ref3 = _trunc_ref(xa, gd)
    P.assert_ulp("aggregate3_density fwd", _n(dens), dens_ref3, K_EXP)
    dens.backward(_t(gd))
    g = _n(X3.grad)[:, 0].reshape(3, n)
    _assert_side("aggregate3_density bwd (current)", g[0], side_ref3 * 0.5)
    _assert_side("aggregate3_density bwd (warped)", g[1], side_ref3 * 0.25)


def test_trunc_exp_clamp_linear(hip_lib):
    """ops.linear(act="trunc_exp") and ops.linear_with_density (emer_linear_fwd epilogue, emer_linear_bwd act' / side
    gradient on column 0): W copies x into column 0, so the pre-activation is exactly x."""
    from emernerf_amd import ops
    x = _clamp_values()
    n = x.size
    gd = np.where(np.arange(n) % 2 == 0, 2.0, -0.5).astype(np.float32)
    dens_ref, side_ref = _trunc_ref(x, gd)
    xin = np.zeros((n, 8), np.float32); xin[:, 0] = x; xin[:, 1] = 1.0
    w = np.zeros((4, 8), np.float32); w[0, 0] = 1.0; w[1, 1] = 1.0; w[2, 0] = 0.5; w[3, 1] = -1.0
    X, W = _t(xin, True), _t(w, True)
    y = ops.linear(X, W, None, "trunc_exp")
    P.assert_ulp("linear trunc_exp fwd", _n(y)[:, 0], dens_ref, K_EXP)
    g = np.zeros((n, 4), np.float32); g[:, 0] = gd
    y.backward(_t(g))
    _assert_side("linear trunc_exp dx", _n(X.grad)[:, 0], side_ref)
    _assert_row_sum("linear trunc_exp dW[0, :2]", _n(W.grad)[0, :2], side_ref[:, None] * xin[:, :2].astype(np.float64))
    assert not _n(W.grad)[1:].any() and not _n(W.grad)[0, 2:].any()
    X2, W2 = _t(xin, True), _t(w, True)
    f, dens = ops.linear_with_density(X2, W2)
    P.assert_exact("linear_with_density feats", _n(f), xin.astype(np.float64) @ w.T.astype(np.float64))
    P.assert_ulp("linear_with_density density", _n(dens), dens_ref, K_EXP)
    dens.backward(_t(gd))
    _assert_side("linear_with_density dx", _n(X2.grad)[:, 0], side_ref)


@pytest.mark.parametrize("fusedw", [True, False])
@pytest.mark.parametrize("which", ["neck", "base_mlp", "density_mlp"])
def test_trunc_exp_clamp_heads(hip_lib, monkeypatch, which, fusedw):
    """fused.neck / base_mlp / density_mlp: layer 0 copies x (+x and -x units), layer 1 reads it back into f0, so f0 = x
    exactly; density and d enc against fp64 around and above the clamp."""
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_WGRAD", fusedw)
    x = _clamp_values()
    reps = 23                                  # 345 rows: several tiles and a ragged tail
    xs = np.tile(x, reps)
    N = xs.size
    gd = np.where(np.arange(N) % 2 == 0, 1.0, -2.0).astype(np.float32)
    dens_ref, side_ref = _trunc_ref(xs, gd)
    L, Fe = 8, 1
    enc = np.zeros((N, 8), np.float32); enc[:, 0] = xs
    w0 = P.positive_copy(64, 8)
    b0 = np.zeros(64, np.float32)
    NG = 1 if which == "density_mlp" else 64
    w1 = np.zeros((NG, 64), np.float32); w1[0, 0] = 1.0; w1[0, 8] = -1.0   # f0 = relu(x) - relu(-x) = x
    b1 = np.zeros(NG, np.float32)
    t = [_t(np.ascontiguousarray(enc.reshape(N, L, Fe).transpose(1, 0, 2)), True)] + [_t(v, True) for v in (w0, b0, w1, b1)]
    if which == "density_mlp":
        dens = fused.density_mlp(*t)
    elif which == "neck":
        _, _, dens = fused.neck(*t)
    else:
        _, dens = fused.base_mlp(*t)
    P.assert_ulp(f"{which} density", _n(dens), dens_ref, K_EXP)
    (dens * _t(gd)).sum().backward()
    denc = _n(t[0].grad)[0, :, 0]
    _assert_side(f"{which} d enc", denc, side_ref)
    # dW1 / db1: sums over the rows of side x h (h = relu(+-x)); row 0 of dW1 and db1 against fp64, every other entry exactly 0
    h = np.maximum(np.stack([xs, -xs], 1).astype(np.float64), 0.0)
    _assert_row_sum(f"{which} dW1[0, (0, 8)]", _n(t[3].grad)[0, [0, 8]], side_ref[:, None] * h)
    _assert_row_sum(f"{which} db1[0]", _n(t[4].grad)[:1], side_ref[:, None])
    assert not np.delete(_n(t[3].grad), [0, 8], axis=1).any() and not _n(t[3].grad)[1:].any() and not _n(t[4].grad)[1:].any()
    assert np.isfinite(_n(t[1].grad)).all(), "weight gradient not finite"


# ------------------------------------------------------------------------------------------ class-default feature heads
def _dino_heads():
    """dino_head Linear(64, 256)-ReLU-Linear(256, 256)-ReLU-Linear(256, 768) and dino_sky_head (dir-PE 27 -> 256 -> 256 ->
    768) as the class builds them (radiance_field.py, the 768-d feature heads)."""
    mk = lambda k: nn.Sequential(nn.Linear(k, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 768))
    return {"dino_head": (mk(64), 64), "dino_sky_head": (mk(27), 27)}


@pytest.mark.parametrize("head", ["dino_head", "dino_sky_head"])
@pytest.mark.parametrize("layer", [0, 1, 2])
@pytest.mark.parametrize("kind", P.KINDS)
def test_feature_head_768_exact(hip_lib, kind, layer, head):
    """The class-default 768-d heads route through radiance_field._run_sequential -> ops.linear (seq_mlp_supported rejects
    768-row weights); forward and every gradient exact with one layer probed."""
    from emernerf_amd import fused
    from emernerf_amd.radiance_field import _run_sequential
    seq, k0 = _dino_heads()[head]
    assert not fused.seq_mlp_supported([m.weight for m in seq if isinstance(m, nn.Linear)])
    widths = (k0, 256, 256, 768)
    N = 517
    x, Ws, Bs = _stack(kind, layer, widths, N, seed=k0 + layer)
    relus = [True, True, False]
    hs, pres = P.mlp_ref(x, Ws, Bs, relus)
    lins = [m for m in seq if isinstance(m, nn.Linear)]
    seq = seq.to(DEV)
    for pas, g in _seeds(kind, N, 768, seed=N + layer).items():
        with torch.no_grad():
            for m, w, b in zip(lins, Ws, Bs):
                m.weight.copy_(_t(w)); m.bias.copy_(_t(b))
        seq.zero_grad(set_to_none=True)
        X = _t(x, True)
        y = _run_sequential(seq, X)
        P.assert_exact(f"{head} {kind} L{layer} fwd", _n(y), hs[-1])
        y.backward(_t(g))
        want = P.mlp_ref_bwd(hs, pres, Ws, relus, g)
        got = {"dx": X.grad}
        for i, m in enumerate(lins):
            got[f"dW{i}"], got[f"db{i}"] = m.weight.grad, m.bias.grad
        _check_grads(f"{head} {kind} layer {layer} pass {pas}", got, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}"))
