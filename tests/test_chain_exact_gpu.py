"""Exact probes of the generic LDS-staged chain kernel (mlp_chain_kernel / emer_mlp_chain) off the 64-wide path.

tests/_chain_probe.py has the argument, the fp64 executor, the launch-plan restatement and the cases;
tests/test_chain_probe_cpu.py proves on the CPU that every probe is inside the exact budget (cover 1.0) and that the cases
reach every branch of the kernel.  Here: (a) descriptors through fused.seg / seg_lm / layer / run_chain, bitwise against the
executor; (b) more rows than one pass of the persistent grid; (c) the non-fast branches of rgb_head, skip_mlp3, base_mlp,
density_mlp and seq_mlp, each with an exact probe per layer and a random-value run through the per-entry bounds of
tests/test_fused_gpu.py; (d) an overflowed density must not reach the next tile of its wave; and the heads too wide for one
chain launch, which run layer by layer.

Not probed exactly: the gradients of the rgb head.  They pass through sigmoid' = out (1 - out), which is on no grid (as
tests/test_head_exact_gpu.py notes for the 64-wide head); the random-value run holds them entry by entry.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _chain_probe as C
from tests import _head_probe as P
from tests._bounds import C_EXP, C_SIG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
E15 = C.E15


def _t(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(DEV)
    return t.requires_grad_(True) if grad else t


def _n(t):
    return t.detach().float().cpu().numpy()


@pytest.fixture
def chain_log(monkeypatch):
    """Records (buf_cols, [(K, N) per layer]) of every chain launch."""
    from emernerf_amd import fused
    log, real = [], fused.run_chain

    def rec(segs, layers, buf_cols, n_rows, ref):
        log.append((buf_cols, [(int(l.K), int(l.N)) for l in layers]))
        return real(segs, layers, buf_cols, n_rows, ref)
    monkeypatch.setattr(fused, "run_chain", rec)
    return log


def _saved_acts(saved, N, H):
    """The stored hidden activations among a Function's saved tensors: contiguous [N, H], in order, each once."""
    out, seen = [], set()
    for t in saved:
        if t is not None and t.dim() == 2 and tuple(t.shape) == (N, H) and t.is_contiguous() and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append(t)
    return out


def _hooks(saved):
    return torch.autograd.graph.saved_tensors_hooks(lambda x: saved.append(x) or x, lambda x: x)


# ------------------------------------------------------------------------------------------ (a) descriptor level
def _check_descriptor(tag, cid, build, kind):
    segs, layers, cols, rows = build(kind)
    ref = C.accumulate_units(segs, layers, cols, rows, C.run_ref(segs, layers, cols, rows))
    got = C.run_gpu(segs, layers, cols, rows)
    cover = {}
    for name in [k for k in ref if ":" not in k]:
        if cid == "sigmoid":
            P.assert_exact(f"{tag} {name} (probe)", ref[name + ":pre"], ref[name + ":pre"], ref[name + ":units"])
            P.assert_ulp(f"{tag} {name}", got[name], ref[name], C_SIG)
        elif cid == "trunc_exp":
            P.assert_exact(f"{tag} {name} (probe)", ref[name + ":pre"], ref[name + ":pre"], ref[name + ":units"])
            P.assert_ulp(f"{tag} {name}", got[name], ref[name], C_EXP)
        else:
            cover[name] = P.assert_exact(f"{tag} {name}", got[name], ref[name], None if cid == "fix" else ref[name + ":units"])
    for key in [k for k in ref if k.endswith(":exp0")]:
        P.assert_ulp(f"{tag} {key}", got[key], C._act(C.ACT_TRUNC_EXP, ref[key]), C_EXP)
    print(f"\n[chain exact] {tag}: cover {cover}")
    return got


@pytest.mark.parametrize("cid", list(C.descriptor_cases()))
@pytest.mark.parametrize("kind", P.KINDS)
def test_descriptor_exact(hip_lib, kind, cid):
    got = _check_descriptor(f"{cid} {kind}", cid, C.descriptor_cases()[cid], kind)
    if cid == "ld_window":   # the columns of the store target past the window are not written
        assert np.isnan(got["y:full"][:, 68:]).all() and not np.isnan(got["y:full"][:, :68]).any()


# ------------------------------------------------------------------------------------------ (b) more than one pass
@pytest.mark.parametrize("cid", list(C.second_pass_cases()))
@pytest.mark.parametrize("kind", P.KINDS)
def test_second_pass_exact(hip_lib, kind, cid):
    build = C.second_pass_cases()[cid]
    segs, layers, cols, rows = build(kind)
    pl = C.plan_of(segs, layers, cols)
    assert rows == pl["rows_per_pass"] + 17 and (pl["n_waves"] == 16) == (cid == "narrow")
    _check_descriptor(f"second pass {cid} {kind} ({pl['n_waves']} waves, {rows} rows)", cid, build, kind)


# ------------------------------------------------------------------------------------------ (c) rgb head
def _rgb_fast(H, NG, Cc, Kh, S, g):
    return H == 64 and NG == 64 and Cc == 3 and Kh <= 64 and S % 16 == 0 and g.stride(0) % 4 == 0 and g.data_ptr() % 16 == 0


def _unaligned(x, grad=False):
    """x [N, NG] as the columns 1 .. NG of a wider tensor: row pitch NG + 3, first element 4 bytes past a 16-byte boundary."""
    wide = torch.zeros((x.shape[0], x.shape[1] + 3), device=DEV)
    wide[:, 1:1 + x.shape[1]] = _t(x)
    wide.requires_grad_(grad)
    return wide, wide[:, 1:1 + x.shape[1]]


@pytest.mark.parametrize("case", C.RGB_CASES, ids=lambda c: "H{}Kh{}NG{}C{}R{}S{}".format(*c))
@pytest.mark.parametrize("probed", [0, 1, 2])
@pytest.mark.parametrize("kind", P.KINDS)
def test_rgb_head_generic_exact(hip_lib, chain_log, kind, probed, case):
    """fused.rgb_head off its fast predicate: a1 and a2 exact, the colours within C_SIG u of sigmoid of the exact pre-activation."""
    from emernerf_amd import fused
    H, Kh, NG, Cc, R, S = case
    N = R * S
    _, _, x = C.rgb_rows(kind, R, S, Kh, NG, seed=H + Kh)
    x, ws = C.skip_probe(kind, probed, H, Kh + NG, Cc, N, seed=H + Kh + probed, x=x)
    xr, xg = x[::S, :Kh], x[:, Kh:]
    assert np.array_equal(np.repeat(xr, S, 0), x[:, :Kh])
    ref = C.skip_ref(x, ws)
    _, geo = _unaligned(xg, True)
    assert not _rgb_fast(H, NG, Cc, Kh, S, geo)
    saved = []
    with _hooks(saved):
        rgb = fused.rgb_head(_t(xr, True), geo, S, *[_t(v, True) for v in ws])
    on_chain = fused.rgb_head_supported(H, Kh, NG, Cc)
    assert [c for c in chain_log] == ([fused.rgb_head_chain_shapes(H, Kh, NG, Cc)[0]] if on_chain else [])
    a = _saved_acts(saved, N, H)
    assert len(a) >= 2
    c1 = P.assert_exact(f"rgb {kind} probed {probed} a1", _n(a[0]), ref["a1"])
    c2 = P.assert_exact(f"rgb {kind} probed {probed} a2", _n(a[1]), ref["a2"])
    P.assert_ulp(f"rgb {kind} probed {probed} colour", _n(rgb), 1.0 / (1.0 + np.exp(-ref["z"])), C_SIG)
    print(f"\n[chain exact] rgb_head {case} {kind} layer {probed} chain={on_chain}: cover a1 {c1} a2 {c2}")


@pytest.mark.parametrize("case", C.RGB_CASES, ids=lambda c: "H{}Kh{}NG{}C{}R{}S{}".format(*c))
def test_rgb_head_generic_bounds(hip_lib, chain_log, case):
    """Random values through skip3_bound of tests/test_fused_gpu.py (its constants), forward and every gradient."""
    from emernerf_amd import fused
    from tests.test_fused_gpu import skip3_bound
    H, Kh, NG, Cc, R, S = case
    N, K0 = R * S, Kh + NG
    g = torch.Generator().manual_seed(N + Kh + H)
    hray, geo = torch.randn(R, Kh, generator=g), torch.randn(N, NG, generator=g)
    Ws = [torch.randn(H, K0, generator=g) / K0 ** 0.5, torch.randn(H, generator=g) * 0.1,
          torch.randn(H, H + K0, generator=g) / (H + K0) ** 0.5, torch.randn(H, generator=g) * 0.1,
          torch.randn(Cc, H, generator=g) / H ** 0.5, torch.randn(Cc, generator=g) * 0.1]
    hd = hray.to(DEV).requires_grad_(True)
    wide, gv = _unaligned(geo.numpy(), True)
    assert not _rgb_fast(H, NG, Cc, Kh, S, gv)
    wd = [w.to(DEV).requires_grad_(True) for w in Ws]
    rgb = fused.rgb_head(hd, gv, S, *wd)
    go = torch.randn(N, Cc, generator=g)
    (rgb * go.to(DEV)).sum().backward()
    on_chain = fused.rgb_head_supported(H, Kh, NG, Cc)
    assert chain_log == (fused.rgb_head_chain_shapes(H, Kh, NG, Cc) if on_chain else [])
    inp = torch.cat([hray.double().repeat_interleave(S, dim=0), geo.double()], -1)
    got = {"out": rgb, "dhray": hd.grad, "dgeo": wide.grad[:, 1:1 + NG]}
    got.update({f"{k}{i}": wd[2 * i + j].grad for i in range(3) for j, k in enumerate(("dW", "db"))})
    skip3_bound(f"rgb_head generic {case}", inp, Ws, go.double(), True, got, per_ray=S, kh=Kh)
    assert not wide.grad[:, 0].any() and not wide.grad[:, 1 + NG:].any()


# ------------------------------------------------------------------------------------------ (c) skip_mlp3
@pytest.mark.parametrize("case", C.SKIP_CASES, ids=lambda c: "H{}K{}C{}N{}".format(*c))
@pytest.mark.parametrize("probed", [0, 1, 2])
@pytest.mark.parametrize("kind", P.KINDS)
def test_skip_mlp3_generic_exact(hip_lib, chain_log, kind, probed, case):
    """fused.skip_mlp3 off its fast predicate, no final activation: a1, a2 and the output exact; pass A: dx exact on every row;
    pass B: the probed layer's dW / db exact, the others where the reference marks them; with the sigmoid the output within
    C_SIG u."""
    from emernerf_amd import fused, _lib
    H, K0, Cc, rows = case
    assert not (H == 64 and K0 <= 64 and Cc <= 16)
    x, ws = C.skip_probe(kind, probed, H, K0, Cc, rows, seed=H + K0 + probed)
    from tests.test_head_exact_gpu import _check_grads, _seeds
    ref = C.skip_ref(x, ws)
    on_chain = fused.skip_mlp3_supported(H, K0, Cc)
    for pas, g in _seeds(kind, rows, Cc, rows + probed).items():
        bw = C.skip_ref_bwd(x, ws, ref, g)
        X, saved, wt = _t(x, True), [], [_t(v, True) for v in ws]
        del chain_log[:]
        with _hooks(saved):
            out = fused.skip_mlp3(X, *wt, final_act=_lib.ACT_NONE)
        a = _saved_acts(saved, rows, H)
        cov = {"a1": P.assert_exact(f"skip {kind} a1", _n(a[0]), ref["a1"]), "a2": P.assert_exact(f"skip {kind} a2", _n(a[1]), ref["a2"]),
               "out": P.assert_exact(f"skip {kind} out", _n(out), ref["z"])}
        out.backward(_t(g))
        assert chain_log == (fused.skip_mlp3_chain_shapes(H, K0, Cc) if on_chain else [])
        want = {k: v for k, v in bw.items() if k[:2] in ("dW", "db")}
        want["dx"] = (bw["dx"], np.broadcast_to(bw["ok"][:, None], bw["dx"].shape))
        got = {"dx": X.grad}
        got.update({f"{n}{i}": wt[2 * i + j].grad for i in range(3) for j, n in enumerate(("dW", "db"))})
        _check_grads(f"skip_mlp3 generic {case} {kind} layer {probed} chain={on_chain} pass {pas}", got, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{probed}", f"db{probed}"))
    sig = fused.skip_mlp3(_t(x), *[_t(v) for v in ws], final_act=_lib.ACT_SIGMOID)
    P.assert_ulp(f"skip {kind} sigmoid", _n(sig), 1.0 / (1.0 + np.exp(-ref["z"])), C_SIG)
    print(f"\n[chain exact] skip_mlp3 {case} {kind} layer {probed} chain={on_chain}: cover {cov}")


@pytest.mark.parametrize("case", C.SKIP_CASES, ids=lambda c: "H{}K{}C{}N{}".format(*c))
@pytest.mark.parametrize("act", ["sigmoid", "none"])
def test_skip_mlp3_generic_bounds(hip_lib, case, act):
    from emernerf_amd import fused, _lib
    from tests.test_fused_gpu import skip3_bound
    H, K0, Cc, N = case
    g = torch.Generator().manual_seed(N + K0 + H)
    vals = [torch.randn(N, K0, generator=g), torch.randn(H, K0, generator=g) / K0 ** 0.5, torch.randn(H, generator=g) * 0.1,
            torch.randn(H, H + K0, generator=g) / (H + K0) ** 0.5, torch.randn(H, generator=g) * 0.1,
            torch.randn(Cc, H, generator=g) / H ** 0.5, torch.randn(Cc, generator=g) * 0.1]
    t = [v.to(DEV).requires_grad_(True) for v in vals]
    out = fused.skip_mlp3(*t, final_act=_lib.ACT_SIGMOID if act == "sigmoid" else _lib.ACT_NONE)
    w = torch.randn(N, Cc, generator=g)
    (out * w.to(DEV)).sum().backward()
    skip3_bound(f"skip_mlp3 generic {case} {act}", vals[0].double(), vals[1:], w.double(), act == "sigmoid",
                dict(zip(("out", "dx", "dW0", "db0", "dW1", "db1", "dW2", "db2"), [out] + [v.grad for v in t])))


# ------------------------------------------------------------------------------------------ (c) base_mlp / density_mlp
def _lm(x, L, Fe):
    return np.ascontiguousarray(x.reshape(x.shape[0], L, Fe).transpose(1, 0, 2))


@pytest.mark.parametrize("case", C.BASE_CASES, ids=lambda c: "L{}F{}H{}NG{}N{}".format(*c))
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("kind", P.KINDS)
def test_base_mlp_generic_exact(hip_lib, chain_log, kind, layer, case):
    """fused.base_mlp on shapes the register-resident neck rejects: features and the stored hidden layer exact, the density
    within C_EXP u; pass A: d enc exact; pass B: the probed layer's dW / db (emer_wgrad_segmented) exact."""
    from emernerf_amd import fused
    from tests.test_head_exact_gpu import _check_grads, _seeds, _stack, _trunc_ref
    L, Fe, H, NG, N = case
    K0 = L * Fe
    assert not fused.neck_supported(L, Fe, H, NG) and fused.base_mlp_supported(K0, H, NG)
    x, Ws, Bs = _stack(kind, layer, (K0, H, NG), N, seed=K0 + H + NG + layer)
    hs, pres = P.mlp_ref(x, Ws, Bs, [True, False])
    for pas, g in _seeds(kind, N, NG, seed=N + layer).items():
        t = [_t(_lm(x, L, Fe), True)] + [_t(v, True) for v in (Ws[0], Bs[0], Ws[1], Bs[1])]
        saved = []
        del chain_log[:]
        with _hooks(saved):
            feats, dens = fused.base_mlp(*t)
        P.assert_exact(f"base {kind} L{layer} feats", _n(feats), hs[-1])
        if H != NG:
            P.assert_exact(f"base {kind} L{layer} h", _n(_saved_acts(saved, N, H)[0]), hs[1])
        P.assert_ulp(f"base {kind} L{layer} density", _n(dens), _trunc_ref(hs[-1][:, 0], 0.0)[0], C_EXP)
        (feats * _t(g)).sum().backward()
        assert chain_log == fused.base_mlp_chain_shapes(K0, H, NG)
        want = P.mlp_ref_bwd(hs, pres, Ws, [True, False], g)
        denc = _n(t[0].grad).transpose(1, 0, 2).reshape(N, K0)
        _check_grads(f"base_mlp generic {case} {kind} layer {layer} pass {pas}",
                     {"dx": torch.from_numpy(denc), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad}, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}"))


@pytest.mark.parametrize("case", C.BASE_CASES, ids=lambda c: "L{}F{}H{}NG{}N{}".format(*c))
def test_base_and_density_mlp_generic_bounds(hip_lib, case):
    """Random values through neck_bound of tests/test_fused_gpu.py: base_mlp (features and density both carry gradient) and
    density_mlp with the same hidden width."""
    from emernerf_amd import fused
    from tests.test_fused_gpu import _lm_rows, neck_bound
    L, Fe, H, NG, N = case
    K0 = L * Fe
    g = torch.Generator().manual_seed(L + NG + N + H)
    enc = torch.randn(L, N, Fe, generator=g)
    x = enc.double().permute(1, 0, 2).reshape(N, K0)
    W0, b0 = torch.randn(H, K0, generator=g) / K0 ** 0.5, torch.randn(H, generator=g) * 0.1
    W1, b1 = torch.randn(NG, H, generator=g) / H ** 0.5, torch.randn(NG, generator=g) * 0.1
    t = [v.to(DEV).requires_grad_(True) for v in (enc, W0, b0, W1, b1)]
    feats, dens = fused.base_mlp(*t)
    gf, gd = torch.randn(N, NG, generator=g), torch.randn(N, generator=g)
    (feats * gf.to(DEV)).sum().add((dens * gd.to(DEV)).sum()).backward()
    neck_bound(f"base_mlp generic {case}", x, W0, b0, W1, b1, gf.double(), gd.double(),
               {"feats": feats, "density": dens, "dx": _lm_rows(t[0].grad, N), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad,
                "db1": t[4].grad})
    assert not fused.neck_supported(L, Fe, H, 1) and fused.density_mlp_supported(K0, H)
    W1d, b1d = torch.randn(1, H, generator=g) / H ** 0.5, torch.randn(1, generator=g) * 0.1
    t = [v.to(DEV).requires_grad_(True) for v in (enc, W0, b0, W1d, b1d)]
    dens = fused.density_mlp(*t)
    (dens * gd.to(DEV)).sum().backward()
    neck_bound(f"density_mlp generic {case}", x, W0, b0, W1d, b1d, torch.zeros(N, 1, dtype=torch.float64), gd.double(),
               {"density": dens, "dx": _lm_rows(t[0].grad, N), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad})


@pytest.mark.parametrize("case", C.BASE_CASES, ids=lambda c: "L{}F{}H{}NG{}N{}".format(*c))
@pytest.mark.parametrize("kind", P.KINDS)
def test_density_mlp_generic_exact(hip_lib, chain_log, kind, case):
    """fused.density_mlp's chain branch, the probe of tests/test_head_exact_gpu.py::test_density_mlp_exact at other hidden
    widths: layer 0 is the probe, unit j is read back as f0 = 32 h_j + 16, so the rows with h_j > 0 lie above the clamp and
    their side gradient is gd fp32(e^15) exactly.  The hidden layer exact, the density within C_EXP u, d enc exact on EVERY row
    (one product per entry), db0 / db1 (and dW0 for "lh") exact with gd on one row."""
    from emernerf_amd import fused
    from tests.test_head_exact_gpu import _check_grads, _trunc_ref
    L, Fe, H, _, N = case
    K0 = L * Fe
    assert not fused.neck_supported(L, Fe, H, 1)
    w0, x, b0, _, _ = P.probe(kind, H, K0, N, seed=K0 + N + H)
    j = 5
    w0[j] = 0.0
    w0[j, [0, 1]] = [1.0, -1.0]
    b0[j] = 0.5
    w1 = np.zeros((1, H), np.float32); w1[0, j] = 32.0
    b1 = np.array([16.0], np.float32)
    hs, pres = P.mlp_ref(x, [w0, w1], [b0, b1], [True, False])
    f0 = hs[-1][:, 0]
    clamped = f0 - 1.0 > 15.0
    assert 0.2 < clamped.mean() < 1.0 and (hs[1][:, j] > 0).sum() == clamped.sum(), "probe broken: clamped fraction"
    rows = np.flatnonzero(clamped & (x != 0).any(1))
    gd_all = np.where(np.arange(N) % 3 == 0, -0.5, 0.5).astype(np.float32)
    passes = {"all rows": gd_all}
    for r in (rows[0], rows[len(rows) // 2], rows[-1]):
        passes[f"row {r}"] = np.where(np.arange(N) == r, gd_all, 0.0).astype(np.float32)
    for name, gd in passes.items():
        t = [_t(_lm(x, L, Fe), True)] + [_t(v, True) for v in (w0, b0, w1, b1)]
        saved = []
        del chain_log[:]
        with _hooks(saved):
            dens = fused.density_mlp(*t)
        P.assert_exact(f"density {kind} h", _n(_saved_acts(saved, N, H)[0]), hs[1])
        P.assert_ulp(f"density {kind}", _n(dens), _trunc_ref(f0, 0.0)[0], C_EXP)
        (dens * _t(gd)).sum().backward()
        assert chain_log == fused.density_mlp_chain_shapes(K0, H)
        side = gd * np.where(clamped, E15, np.exp(np.minimum(f0 - 1.0, 15.0)))
        want = P.mlp_ref_bwd(hs, pres, [w0, w1], [True, False], side[:, None], row_ok=clamped | (gd == 0))
        must = () if name == "all rows" else ("db0", "db1") + (("dW0",) if kind == "lh" else ())
        denc = _n(t[0].grad).transpose(1, 0, 2).reshape(N, K0)
        if name == "all rows":
            P.assert_exact(f"density generic {case} {kind} d enc", denc, (32.0 * side * clamped)[:, None] * w0[j].astype(np.float64)[None, :])
            assert np.count_nonzero(denc) >= clamped.sum()
        got = {"dx": torch.from_numpy(denc), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad}
        _check_grads(f"density_mlp generic {case} {kind} gd on {name}", got, want, must_cover=must)
        for m in must:
            assert np.count_nonzero(want[m][0]) >= 1, f"probe broken: {m} has no non-zero entry"


# ------------------------------------------------------------------------------------------ (c) seq_mlp
@pytest.mark.parametrize("widths,layer", [(w, i) for w in C.SEQ_CASES for i in range(len(w) - 1)])
@pytest.mark.parametrize("kind", P.KINDS)
def test_seq_mlp_generic_exact(hip_lib, chain_log, kind, widths, layer):
    """fused.seq_mlp off the register-resident kernels: the output and every stored activation exact, pass A: dx, pass B: the
    probed layer's dW / db.  The stacks of SEQ_CHAIN are one chain launch each way, the others run layer by layer."""
    from emernerf_amd import fused, _lib
    from tests.test_head_exact_gpu import _check_grads, _seeds, _stack
    n, N = len(widths) - 1, C.SEQ_ROWS
    x, Ws, Bs = _stack(kind, layer, widths, N, seed=sum(widths) + layer)
    relus = [True] * (n - 1) + [False]
    hs, pres = P.mlp_ref(x, Ws, Bs, relus)
    assert not fused.rmlp_supported([torch.empty(w.shape) for w in Ws], widths[0], 0)
    on_chain = widths in C.SEQ_CHAIN
    assert fused.seq_mlp_supported([torch.empty(w.shape) for w in Ws]) == on_chain
    for pas, g in _seeds(kind, N, widths[-1], seed=N + layer).items():
        X, Wt, Bt = _t(x, True), [_t(w, True) for w in Ws], [_t(b, True) for b in Bs]
        saved = []
        del chain_log[:]
        with _hooks(saved):
            out = fused.seq_mlp(X, Wt, Bt, _lib.ACT_NONE)
        P.assert_exact(f"seq {kind} L{layer} fwd", _n(out), hs[-1])
        for i in range(1, n):   # the stored hidden activations
            a = [t for t in saved if t.dim() == 2 and tuple(t.shape) == (N, widths[i]) and t.data_ptr() != X.data_ptr()]
            assert a and any(np.array_equal(_n(t).astype(np.float64), hs[i]) for t in a), f"seq {kind} L{layer}: hidden {i} not exact"
        out.backward(_t(g))
        assert chain_log == (fused.seq_mlp_chain_shapes(list(widths)) if on_chain else [])
        want = P.mlp_ref_bwd(hs, pres, Ws, relus, g)
        got = {"dx": X.grad}
        for i in range(n):
            got[f"dW{i}"], got[f"db{i}"] = Wt[i].grad, Bt[i].grad
        _check_grads(f"seq_mlp generic {widths} {kind} layer {layer} chain={on_chain} pass {pas}", got, want,
                     must_cover=("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}"))


@pytest.mark.parametrize("dims", C.SEQ_CASES)
@pytest.mark.parametrize("sig", [False, True])
def test_seq_mlp_generic_bounds(hip_lib, dims, sig):
    from emernerf_amd import fused, _lib
    from tests.test_fused_gpu import stack_bound
    N = C.SEQ_ROWS
    g = torch.Generator().manual_seed(sum(dims) + N + 3)
    x = torch.randn(N, dims[0], generator=g)
    n = len(dims) - 1
    Ws = [torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5 for i in range(n)]
    Bs = [torch.randn(dims[i + 1], generator=g) * 0.1 for i in range(n)]
    t = [v.to(DEV).requires_grad_(True) for v in [x] + Ws + Bs]
    out = fused.seq_mlp(t[0], t[1:1 + n], t[1 + n:], _lib.ACT_SIGMOID if sig else _lib.ACT_NONE)
    w = torch.randn(N, dims[-1], generator=g)
    (out * w.to(DEV)).sum().backward()
    got = {"out": out, "dx": t[0].grad}
    got.update({f"dW{i}": t[1 + i].grad for i in range(n)})
    got.update({f"db{i}": t[1 + n + i].grad for i in range(n)})
    stack_bound(f"seq_mlp generic {dims} sig={sig}", x.double(), Ws, Bs, sig, w.double(), got)


# ------------------------------------------------------------------------------------------ (d) the inf hazard
def test_overflowed_density_does_not_reach_the_next_tile(hip_lib):
    """density_mlp's chain branch with H = 20 (H % 8 = 4) at one pass of rows + 17: a third of the first pass's rows have a
    pre-activation of 100 (density inf).  Every row of the second pass must be finite and equal, bit for bit, a launch of
    those rows alone."""
    from emernerf_amd import fused
    L, Fe, H = 7, 1, 20
    assert not fused.neck_supported(L, Fe, H, 1)
    pl = C.plan(*fused.density_mlp_chain_shapes(L * Fe, H)[0])
    first = pl["rows_per_pass"]
    N = first + 17
    rng = np.random.default_rng(3)
    x = (rng.integers(-8, 9, size=(N, L * Fe)) / 8.0).astype(np.float32)
    x[:first, 0] = np.where(np.arange(first) % 3 == 0, 1.0, 0.25)
    x[first:, 0] = 0.5
    w0 = P.positive_copy(H, L * Fe)
    w1 = np.zeros((1, H), np.float32); w1[0, 0] = 100.0; w1[0, 3] = 0.5
    p = [_t(v) for v in (w0, np.zeros(H, np.float32), w1, np.zeros(1, np.float32))]
    with torch.no_grad():
        dens = _n(fused.density_mlp(_t(_lm(x, L, Fe)), *p))
        alone = _n(fused.density_mlp(_t(_lm(x[first:], L, Fe)), *p))
    assert np.isinf(dens[:first][::3]).all() and np.isfinite(dens[:first][1::3]).all(), "probe broken: no overflow in the first pass"
    assert np.isfinite(dens[first:]).all(), f"second pass: {int((~np.isfinite(dens[first:])).sum())} of 17 rows are not finite"
    assert np.array_equal(dens[first:].view(np.uint32), alone.view(np.uint32))
    t = [_t(_lm(x, L, Fe), True)] + [v.clone().requires_grad_(True) for v in p]   # the training forward stores the hidden layer
    d2 = fused.density_mlp(*t)
    assert np.array_equal(_n(d2).view(np.uint32), dens.view(np.uint32))


# ------------------------------------------------------------------------------------------ heads too wide for the chain
def test_wide_heads_run_layer_by_layer(hip_lib, chain_log):
    """A 256-wide rgb head and sky head through RadianceField.query_rgb / query_sky: no chain launch, no error from inside the
    forward, and forward and gradients within skip3_bound."""
    from emernerf_amd.encodings import HashEncoder
    from emernerf_amd.radiance_field import RadianceField
    from tests.test_fused_gpu import skip3_bound
    torch.manual_seed(5)
    rf = RadianceField(HashEncoder(3, 4, 16, 64, 12, 2, verbose=False), geometry_feature_dim=64, head_mlp_layer_width=256,
                       enable_sky_head=True).to(DEV)
    R, S = 9, 24
    g = torch.Generator().manual_seed(11)
    d = F.normalize(torch.randn(R, 3, generator=g), dim=-1).to(DEV)
    dirs = d[:, None, :].expand(R, S, 3)
    geo = torch.randn(R, S, 64, generator=g).to(DEV).requires_grad_(True)
    rgb = rf.query_rgb(dirs, geo)["rgb"]
    sky = rf.query_sky(d)["rgb_sky"]
    go, gs = torch.randn(R * S, 3, generator=g), torch.randn(R, 3, generator=g)
    ((rgb.reshape(-1, 3) * go.to(DEV)).sum() + (sky * gs.to(DEV)).sum()).backward()
    assert chain_log == []
    for head, x, out, gg, extra in ((rf.rgb_head, torch.cat([rf.direction_encoding(d, remap=True).repeat_interleave(S, dim=0), geo.reshape(R * S, 64)], -1),
                                     rgb.reshape(-1, 3), go, {"dgeo": geo.grad.reshape(R * S, 64)}),
                                    (rf.sky_head, rf.direction_encoding(d, remap=False), sky, gs, {})):
        Ws = [p.detach().cpu() for l in head.layers for p in (l.weight, l.bias)]
        got = {"out": out}
        got.update({f"{k}{i}": p.grad for i, l in enumerate(head.layers) for k, p in (("dW", l.weight), ("db", l.bias))})
        got.update(extra)
        kh = x.shape[1] - 64
        skip3_bound(f"wide head {x.shape}", x.detach().double().cpu(), Ws, gg.double(), True, got,
                    per_ray=S if extra else 0, kh=kh if extra else 0)
