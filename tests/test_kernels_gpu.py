"""Kernel-level parity: every C-ABI entry point vs the CPU oracle on seeded inputs (MI355X only).

Tolerances: sampler offsets bit-exact; everything else fp32 with the tolerance written at the check.
Grid kernels in fp32 are also held per entry to c 2^-24 abs_sum of the double-precision oracle (tests/_bounds.py).
"""
import numpy as np
import pytest
import torch

from tests import _composite_probe as CP
from tests import _update_probe as UP
from tests._bounds import (assert_bound, assert_err_bound, c_atomic, c_embed_grad, c_forward, c_input_grad, c_ray_pre_bwd, c_ray_pre_fwd, c_ray_wgrad, c_sliced,
                           contract_bwd_bounds)

pytestmark = pytest.mark.gpu

GRIDS = {
    # name: (D, L, base, max, log2T, F)
    "cfg2_static": (3, 16, 16, 2048, 19, 2),       # HashEncoder defaults, encodings.py:110-118
    "default_static": (3, 10, 16, 8192, 20, 4),    # default_config.yaml:62-69
    "dynamic_xyzt": (4, 10, 32, 8192, 18, 4),      # default_config.yaml:70-77
    "flow_xyzt": (4, 10, 16, 4096, 18, 4),         # radiance_field.py:916-923
    "prop0": (3, 8, 16, 512, 20, 1),               # default_config.yaml:51-58
    "cfg0_static": (3, 4, 16, 2048, 19, 2),        # BASELINE configs[0]: fewer levels than XCDs; level 1 (res 81) barely hashed
    "tiny_f8": (3, 4, 4, 64, 10, 8),
    "tiny_2d": (2, 5, 8, 256, 12, 2),
    # the (D, F) instantiations of dispatch_df that no grid above reaches
    "tiny_2d_f1": (2, 5, 8, 256, 12, 1),
    "tiny_2d_f4": (2, 5, 8, 256, 12, 4),
    "tiny_2d_f8": (2, 5, 8, 256, 12, 8),
    "tiny_4d_f1": (4, 4, 4, 32, 12, 1),            # level 0 (5^4 cells) is dense: the xyzt tables above are hashed from level 0
    "tiny_4d_f2": (4, 4, 4, 32, 12, 2),
    "tiny_4d_f8": (4, 4, 4, 32, 12, 8),
}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _mk(oracle, name):
    from emernerf_amd import _lib
    D, L, base, mx, T, F = GRIDS[name]
    meta = oracle.grid_meta_from_encoder_args(D, L, base, mx, T, F)
    desc = _lib.make_grid_desc(D, L, F, T, base, meta.per_level_scale)
    return meta, desc


def _inputs(meta, n, seed, edge=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, meta.n_dims, generator=g)
    if edge and n >= 8:  # edge cases the reference hits: zeroed rows, values next to 0 and 1
        x[0] = 0.0
        x[1] = 1.0 - 2 ** -24
        x[2] = 2 ** -20
        x[3] = 0.999
        x[4, 0] = 0.9671  # level-0 corner wrap (res 16 -> c = 16)
    p = torch.rand(meta.n_params, generator=g) - 0.5
    return x, p


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_desc_matches_oracle(hip_lib, oracle, name):
    meta, desc = _mk(oracle, name)
    L = meta.n_levels
    assert desc.n_entries == meta.n_entries
    assert np.array_equal(np.array(desc.scale[:L], np.float32).view(np.uint32), meta.scale.view(np.uint32))
    for fld in ("res", "size", "offset", "hashed"):
        assert np.array_equal(np.array(getattr(desc, fld)[:L], np.uint32), getattr(meta, fld))


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_hashgrid_fwd(hip_lib, oracle, name, n):
    from emernerf_amd import ops
    meta, desc = _mk(oracle, name)
    x, p = _inputs(meta, n, 1)
    ref = oracle.hashgrid_fwd(meta, x, p)
    dev = _dev()
    lm = ops.hashgrid_fwd_raw(desc, x.to(dev), p.to(dev), level_major=True)
    rm = ops.hashgrid_fwd_raw(desc, x.to(dev), p.to(dev), level_major=False)
    L, F = meta.n_levels, meta.n_features
    lm_as_rows = lm.permute(1, 0, 2).reshape(n, L * F).cpu().numpy()
    # same fmaf cell + same corner order => only the FMA contraction of acc += w*v may differ
    np.testing.assert_allclose(rm.cpu().numpy(), ref, rtol=0, atol=2e-6)
    np.testing.assert_allclose(lm_as_rows, ref, rtol=0, atol=2e-6)
    ref64, fabs_ = oracle.hashgrid_fwd_bound(meta, x, p)
    assert_bound(rm.cpu().numpy(), ref64, fabs_, c_forward(meta.n_dims), f"fwd {name} n={n} row-major", meta=meta, kind="fwd")
    assert_bound(lm_as_rows, ref64, fabs_, c_forward(meta.n_dims), f"fwd {name} n={n} level-major", meta=meta, kind="fwd")
    tr = ops.layout_transpose(lm, L, n, F, to_row_major=True)
    assert torch.equal(tr, rm)
    back = ops.layout_transpose(tr, L, n, F, to_row_major=False)
    assert torch.equal(back, lm)


@pytest.mark.parametrize("name", ["cfg2_static", "prop0", "default_static", "flow_xyzt", "tiny_2d"])
@pytest.mark.parametrize("half", [False, True])
def test_hashgrid_fwd_is_independent_of_the_launch_size(hip_lib, oracle, name, half):
    """The encoding of 40 000 samples in one launch is BITWISE the concatenation of five 8 000-sample launches (the XCD-aware level map
    and the chunking only move work), its slice bitmaps drive the owner-computes backward to the oracle's table gradient, coordinates
    outside [0, 1] wrap as tcnn's do.  (Written in round 6 for the LDS-staged coarse levels, profiles/r06_fwd_lds_stage.txt: that path
    was bit-identical and lost the A/B; the test stays as a consistency check of the forward.)"""
    from emernerf_amd import ops
    meta, desc = _mk(oracle, name)
    n = 40000
    x, p = _inputs(meta, n, 7)
    x[5] = torch.tensor([1.3, -0.2, 0.5, 0.1][: meta.n_dims])   # outside [0, 1]: the dense index wraps (tcnn does not clamp)
    if half:
        p = p.half()
    dev = _dev()
    xd, pd = x.to(dev), p.to(dev)
    big, masks = ops.hashgrid_fwd_raw(desc, xd, pd, level_major=True, want_masks=True)
    parts = [ops.hashgrid_fwd_raw(desc, xd[i:i + 8000].contiguous(), pd, level_major=True) for i in range(0, n, 8000)]
    assert torch.equal(big, torch.cat(parts, dim=1)), "the encoding depends on how the samples are cut into launches"
    ref = oracle.hashgrid_fwd(meta, x, p.float())
    np.testing.assert_allclose(big.permute(1, 0, 2).reshape(n, -1).cpu().numpy(), ref, rtol=0, atol=2e-6)
    if not half and ops.sliced_supported(desc):
        dout = torch.randn(meta.n_levels, n, meta.n_features, generator=torch.Generator().manual_seed(3)).to(dev)
        import ctypes
        from emernerf_amd import _lib
        g_big = torch.empty(meta.n_params, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.call("emer_hashgrid_bwd_params_sliced", ctypes.byref(desc), ops._ptr(xd), ops._ptr(dout), meta.n_features, n * meta.n_features,
                      ops._ptr(masks), ops._ptr(g_big), n, ops._stream(xd))
        ref_g = oracle.hashgrid_bwd_params(meta, x, dout.permute(1, 0, 2).reshape(n, -1).cpu())
        np.testing.assert_allclose(g_big.cpu().numpy(), ref_g, rtol=0, atol=2e-5 * float(np.abs(ref_g).max()))
        g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout.permute(1, 0, 2).reshape(n, -1).cpu())
        assert_bound(g_big.cpu().numpy(), g64, gabs, c_sliced(meta, desc, hits), f"sliced bwd {name} n={n}", meta=meta, hits=hits)


@pytest.mark.parametrize("name", ["cfg2_static", "dynamic_xyzt", "prop0", "tiny_f8", "tiny_2d"])
def test_hashgrid_fp16_tables(hip_lib, oracle, name):
    from emernerf_amd import ops
    meta, desc = _mk(oracle, name)
    x, p = _inputs(meta, 3000, 2)
    ph = p.half()
    ref = oracle.hashgrid_fwd(meta, x, ph.float())  # oracle on the fp16-rounded table, fp32 accumulate
    dev = _dev()
    out = ops.hashgrid_fwd_raw(desc, x.to(dev), ph.to(dev), level_major=False)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", list(GRIDS))
def test_hashgrid_backward(hip_lib, oracle, name):
    from emernerf_amd import ops
    meta, desc = _mk(oracle, name)
    n = 4099
    x, p = _inputs(meta, n, 3)
    g = torch.Generator().manual_seed(4)
    dout = torch.randn(n, meta.n_output_dims, generator=g)
    dout[5] = 0.0  # exact-zero rows are skipped by the kernel
    ref_dp = oracle.hashgrid_bwd_params(meta, x, dout)
    ref_dx = oracle.hashgrid_bwd_input(meta, x, p, dout)
    dev = _dev()
    xd = x.to(dev).requires_grad_(True)
    pd = p.to(dev).requires_grad_(True)
    out = ops.hashgrid_encode(xd, pd, desc)
    out.backward(dout.to(dev))
    # fp32 atomics in arbitrary order vs double accumulation: error ~ sqrt(k) ulp of the partial sums
    scale = np.abs(ref_dp).max()
    np.testing.assert_allclose(pd.grad.cpu().numpy(), ref_dp, rtol=0, atol=2e-5 * scale)
    sx = np.abs(ref_dx).max()
    np.testing.assert_allclose(xd.grad.cpu().numpy(), ref_dx, rtol=0, atol=2e-5 * sx)
    g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    c = c_sliced(meta, desc, hits) if ops.sliced_supported(desc) else c_atomic(meta.n_dims, hits)
    assert_bound(pd.grad.cpu().numpy(), g64, gabs, c, f"bwd params {name}", meta=meta, hits=hits)
    dx64, bx = oracle.hashgrid_bwd_input_bound(meta, x, p, dout)
    assert_bound(xd.grad.cpu().numpy(), dx64, bx, c_input_grad(meta.n_dims, meta.n_levels, meta.n_features), f"bwd input {name}",
                 meta=meta, kind="dx")


@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("skip", [0, 1500])
def test_hashgrid_input_gradient_from_stored_jacobians(hip_lib, oracle, monkeypatch, name, skip):
    """[r4] ops.hashgrid_encode_lm with positions that need a gradient: the forward stores d out / d x for the rows past
    ``skip_dx_rows`` (emer_hashgrid_fwd_jac) and the backward contracts them with dOut (emer_hashgrid_bwd_input_jac).  The encoding is
    bitwise the plain forward's (the four-feature grids the flow configs differentiate), the input gradient matches the oracle AND the
    gather kernel it replaces, skipped rows get zero."""
    from emernerf_amd import ops
    meta, desc = _mk(oracle, name)
    n = 4099
    x, p = _inputs(meta, n, 13)
    L, F = meta.n_levels, meta.n_features
    dout = torch.randn(n, meta.n_output_dims, generator=torch.Generator().manual_seed(14))
    dev = _dev()
    dlm = dout.view(n, L, F).permute(1, 0, 2).contiguous().to(dev)
    got = {}
    for jac in (True, False):
        monkeypatch.setattr(ops, "GRID_JAC", jac)
        xd = x.to(dev).requires_grad_(True)
        pd = p.to(dev).requires_grad_(True)
        lm = ops.hashgrid_encode_lm(xd, pd, desc, skip_dx_rows=skip)
        lm.backward(dlm)
        got[jac] = (lm.detach().clone(), xd.grad.clone(), pd.grad.clone())
    if F * 4 > 16:   # (entries of <= 16 bytes [r6: incl. F = 4]: the plain forward takes its paired-gather path on hashed levels, the Jacobian forward the
        assert torch.equal(got[True][0], got[False][0]), "the Jacobian forward must not change the encoding"   # generic loop)
    else:
        np.testing.assert_allclose(got[True][0].cpu().numpy(), got[False][0].cpu().numpy(), rtol=0, atol=1e-6)
    gp = got[False][2].abs().max().item()   # (two launches of the owner-computes backward agree to an ulp or two, not bitwise)
    assert (got[True][2] - got[False][2]).abs().max().item() <= 1e-6 * gp
    ref_dx = oracle.hashgrid_bwd_input(meta, x, p, dout)
    ref_dx[:skip] = 0.0
    sx = np.abs(ref_dx).max()
    np.testing.assert_allclose(got[True][1].cpu().numpy(), ref_dx, rtol=0, atol=2e-5 * sx)
    np.testing.assert_allclose(got[True][1].cpu().numpy(), got[False][1].cpu().numpy(), rtol=0, atol=2e-6 * sx)
    dx64, bx = oracle.hashgrid_bwd_input_bound(meta, x, p, dout)
    dx64[:skip] = 0.0   # skipped rows: zero bound, so exactly zero
    bx[:skip] = 0.0
    for jac in (True, False):
        assert_bound(got[jac][1].cpu().numpy(), dx64, bx, c_input_grad(meta.n_dims, L, F), f"input grad {name} skip={skip} jac={jac}",
                     meta=meta, kind="dx")


@pytest.mark.parametrize("name", ["cfg2_static", "default_static", "dynamic_xyzt", "flow_xyzt", "prop0", "cfg0_static"])
@pytest.mark.parametrize("layout", ["point", "point_sparse", "shuffled", "cell_sorted", "lattice", "box", "ragged", "dead_rays"])
def test_hashgrid_sliced_layouts_small(hip_lib, oracle, name, layout):
    """The owner-computes backward on the sample layouts of tests/test_a_metric_shape_gpu.layout_inputs at 20 000 samples (ragged:
    1, 63 and 65 samples -- a partial last bitmap word, trip and workgroup), every table entry within the per-entry bound of
    tests/_bounds.py; three layouts also through the level-range split and through sliced + sliced_add."""
    from tests.test_a_metric_shape_gpu import layout_inputs, sliced_layout_check
    meta, desc = _mk(oracle, name)
    for n in ((1, 63, 65) if layout == "ragged" else (20000,)):
        x, dout = layout_inputs(layout, meta, n, seed=43 + n)
        sliced_layout_check(oracle, meta, desc, name, layout, x, dout)
        if layout in ("point_sparse", "cell_sorted", "dead_rays"):
            sliced_layout_check(oracle, meta, desc, name, layout, x, dout, route="split")
            sliced_layout_check(oracle, meta, desc, name, layout, x, dout, route="add")


def test_hashgrid_fp16_grads(hip_lib, oracle):
    from emernerf_amd import ops
    meta, desc = _mk(oracle, "cfg2_static")
    n = 2048
    x, p = _inputs(meta, n, 5)
    dout = torch.randn(n, meta.n_output_dims, generator=torch.Generator().manual_seed(6)) * 1e-2
    ref = oracle.hashgrid_bwd_params(meta, x, dout)
    dev = _dev()
    pd = p.to(dev).requires_grad_(True)
    out = ops.hashgrid_encode(x.to(dev), pd, desc, grad_dtype=torch.float16)
    out.backward(dout.to(dev))
    got = pd.grad.cpu().numpy()
    # half2 atomics: each add rounds to fp16 (rel 2^-11); stated deviation from the fp32 path
    assert np.abs(got - ref).max() <= 4e-3 * np.abs(ref).max() + 1e-6


def test_hashgrid_errors(hip_lib):
    from emernerf_amd import _lib
    with pytest.raises(_lib.EmerError):
        _lib.make_grid_desc(5, 4, 2, 19, 16, 1.5)
    with pytest.raises(_lib.EmerError):
        _lib.make_grid_desc(3, 4, 3, 19, 16, 1.5)


@pytest.mark.parametrize("R,m,n", [(1, 2, 128), (37, 129, 64), (64, 65, 128), (5, 2, 1), (9, 300, 257)])
@pytest.mark.parametrize("stratified", [False, True])
def test_importance_sample_bit_exact(hip_lib, oracle, R, m, n, stratified):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(R * 1000 + m)
    w = torch.rand(R, m - 1, generator=g) ** 4  # peaky histograms
    w[0, : (m - 1) // 2] = 0.0  # flat CDF stretch (delta < 1e-10 branch)
    cdf = torch.cat([torch.zeros(R, 1), torch.cumsum(w, -1)], -1)
    cdf = cdf / cdf[:, -1:].clamp_min(1e-12)
    if R > 2:
        cdf[2] = cdf[2] * 0.6 + 0.1  # cdf_first != 0, cdf_last != 1
    vals = torch.sort(torch.rand(R, m, generator=g), -1).values
    jit = torch.rand(R, generator=g) if stratified else None
    ref = oracle.importance_sample(vals, cdf, n, jit)
    ref_t = oracle.stot(ref, 0.1, 1000.0, "uniform_lindisp")
    dev = _dev()
    s, t = ops.importance_sample(vals.to(dev), cdf.to(dev), n, None if jit is None else jit.to(dev),
                                 stot=(0.1, 1000.0, "uniform_lindisp"))
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref.view(np.uint32)), "sample offsets must be bit-exact"
    assert np.array_equal(t.cpu().numpy().view(np.uint32), ref_t.view(np.uint32)), "s->t must be bit-exact"
    assert (np.diff(ref, axis=-1) >= 0).all()
    from tests import _sample_probe as SP
    for typ in ("uniform", "lindisp", "uniform_lindisp", "sqrt", "log", "uniform_lindisp_0"):
        a = ops.stot(s, 0.5, 300.0, typ).cpu().numpy()
        if typ == "log":     # the device library's expf: tests/_sample_probe.LOG_ULP_DEVICE
            SP.check_log(f"stot log R={R} m={m} n={n}", a, SP.stot_arg("log", ref, 0.5, 300.0), SP.LOG_ULP_DEVICE)
        else:
            assert np.array_equal(a.view(np.uint32), oracle.stot(ref, 0.5, 300.0, typ).view(np.uint32)), typ


def test_importance_sample_end_clamp_bit_exact(hip_lib, oracle):
    """Stratified offset 1 - 2^-24 on a CDF with a saturated tail: u_n == cdf_last, the search runs off the row and both kernels
    return the LAST edge (nerfacc's separate p0 / p1 clamps), bit for bit the oracle."""
    from emernerf_amd import ops
    from tests.test_oracle_cpu import _end_clamp_case
    vals, cdf, n, jit = _end_clamp_case()
    ref = oracle.importance_sample(vals, cdf, n, jit)
    dev = _dev()
    stot = (0.1, 1000.0, "uniform_lindisp")
    s, t = ops.importance_sample(vals.to(dev), cdf.to(dev), n, jit.to(dev), stot=stot)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(s[:, -1].cpu().numpy(), vals[:, -1].numpy()), "u >= cdf_last must return the last edge"
    o = torch.rand(3, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(3, 3, generator=torch.Generator().manual_seed(2)), dim=-1).to(dev)
    aabb = torch.tensor([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0], device=dev)
    out = ops.importance_sample(vals.to(dev), cdf.to(dev), n, jit.to(dev), stot=stot, intervals=True, points=(o, d, aabb, True, False))
    assert torch.equal(out[0], s), "the fused sampler + points kernel takes the same end clamp"


def _torch_render(ts, te, sg):
    sdt = sg * (te - ts)
    cum = torch.cumsum(sdt, -1)
    excl = torch.cat([torch.zeros_like(cum[:, :1]), cum[:, :-1]], -1)
    T = torch.exp(-excl)
    a = 1 - torch.exp(-sdt)
    return T * a, T, a


def test_importance_sample_interval_outputs(hip_lib):
    """intervals=True: the kernel's (t_starts, t_ends) are bit-identical to slicing its edge output."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    R, m, n = 37, 65, 128
    vals = torch.sort(torch.rand(R, m, generator=g), -1).values
    cdf = torch.cumsum(torch.rand(R, m, generator=g), -1)
    cdf = (cdf - cdf[:, :1]) / (cdf[:, -1:] - cdf[:, :1])
    jit = torch.rand(R, generator=g)
    stot = (0.1, 1000.0, "uniform_lindisp")
    s0, t = ops.importance_sample(vals.to(dev), cdf.to(dev), n, jit.to(dev), stot=stot)
    s1, ts, te = ops.importance_sample(vals.to(dev), cdf.to(dev), n, jit.to(dev), stot=stot, intervals=True)
    assert torch.equal(s0, s1) and ts.is_contiguous() and te.is_contiguous()
    assert torch.equal(ts, t[:, :-1]) and torch.equal(te, t[:, 1:])


@pytest.mark.parametrize("R,S", [(1, 1), (3, 64), (50, 128), (7, 130), (4, 333)])
def test_render_weights(hip_lib, oracle, R, S):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(R + S)
    edges = torch.sort(torch.rand(R, S + 1, generator=g) * 50 + 0.1, -1).values
    ts, te = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    sg = torch.rand(R, S, generator=g) ** 3 * 2.0
    w_ref, T_ref, a_ref = oracle.render_weights(ts, te, sg)
    dev = _dev()
    sgd = sg.to(dev).requires_grad_(True)
    w, T, a, cdfs, stats = ops.render_weights(ts.to(dev), te.to(dev), sgd)
    np.testing.assert_allclose(w.detach().cpu().numpy(), w_ref, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(T.detach().cpu().numpy(), T_ref, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(a.detach().cpu().numpy(), a_ref, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(cdfs.detach().cpu().numpy()[:, :S], 1 - T_ref, rtol=0, atol=2e-6)
    assert (cdfs.detach().cpu().numpy()[:, S] == 1.0).all()
    mid = ((ts + te) / 2).numpy()
    np.testing.assert_allclose(stats[:, 0].detach().cpu().numpy(), w_ref.sum(-1), rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(stats[:, 1].detach().cpu().numpy(), (w_ref * mid).sum(-1), rtol=2e-5, atol=1e-5)
    # median depth (render_utils.py:107-115); tolerate a one-sample slip when cumsum sits on 0.5
    cw = np.cumsum(w_ref, -1)
    idx = np.minimum((cw < 0.5).sum(-1), S - 1)
    med = stats[:, 2].detach().cpu().numpy()
    ok = [np.isclose(med[r], mid[r, max(idx[r] - 1, 0):idx[r] + 2], rtol=1e-6).any() for r in range(R)]
    assert all(ok)
    # backward through weights, trans, cdfs and the per-ray sums vs torch autograd (fp64 on CPU)
    gw, gT, gc = (torch.randn(R, S, generator=g), torch.randn(R, S, generator=g), torch.randn(R, S + 1, generator=g))
    gs = torch.randn(R, 2, generator=g)
    ga = torch.randn(R, S, generator=g)  # alphas is a differentiable output too (the reference forms trans * alphas itself)
    loss = (w * gw.to(dev)).sum() + (T * gT.to(dev)).sum() + (cdfs * gc.to(dev)).sum() + (stats[:, :2] * gs.to(dev)).sum() \
        + (a * ga.to(dev)).sum()
    loss.backward()
    s64 = sg.double().requires_grad_(True)
    w2, T2, a2 = _torch_render(ts.double(), te.double(), s64)
    c2 = 1 - torch.cat([T2, torch.zeros(R, 1, dtype=torch.double)], -1)
    st2 = torch.stack([w2.sum(-1), (w2 * (ts + te).double() / 2).sum(-1)], -1)
    ((w2 * gw).sum() + (T2 * gT).sum() + (c2 * gc).sum() + (st2 * gs).sum() + (a2 * ga).sum()).backward()
    ref_g = s64.grad.numpy()
    np.testing.assert_allclose(sgd.grad.cpu().numpy(), ref_g, rtol=1e-4, atol=1e-5 * np.abs(ref_g).max())
    # every entry inside its first-order fp64 bound (tests/_bounds.py render_bounds, dsigma_bound); the median exact except on
    # a ray whose cumsum of w comes within its bound of 0.5
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    p = dict(ts=ts.numpy(), te=te.numpy(), sg=sg.numpy(), dW=gw.numpy(), dT=gT.numpy(), dA=ga.numpy(), dC=gc.numpy(),
             dS=torch.cat([gs, torch.zeros(R, 2)], -1).numpy())
    CP.check_real_render(p, dict(weights=n(w), trans=n(T), alphas=n(a), cdfs=n(cdfs), stats=n(stats), d_sigma=n(sgd.grad)),
                         f"render_weights R={R} S={S}", allow_ambiguous=True)


@pytest.mark.parametrize("C", [None, 1, 3, 6, 64, 100])
def test_accumulate(hip_lib, oracle, C):
    from emernerf_amd import ops
    R, S = 33, 128
    g = torch.Generator().manual_seed(7)
    w = torch.rand(R, S, generator=g)
    v = None if C is None else torch.randn(R, S, C, generator=g)
    ref = oracle.accumulate(w, v)
    dev = _dev()
    wd = w.to(dev).requires_grad_(True)
    vd = None if v is None else v.to(dev).requires_grad_(True)
    out = ops.accumulate_along_rays(wd, vd)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref, rtol=1e-5, atol=1e-5)
    go = torch.randn(out.shape, generator=g)
    out.backward(go.to(dev))
    if v is None:
        np.testing.assert_allclose(wd.grad.cpu().numpy(), go.expand(R, S).numpy(), rtol=1e-6)
    else:
        np.testing.assert_allclose(wd.grad.cpu().numpy(), torch.einsum("rc,rsc->rs", go, v).numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(vd.grad.cpu().numpy(), (w[..., None] * go[:, None, :]).numpy(), rtol=1e-6, atol=1e-7)
    CP.check_real_accumulate(dict(w=w.numpy(), v=None if v is None else v.numpy(), go=go.numpy()), out.detach().cpu().numpy(),
                             wd.grad.cpu().numpy(), None if v is None else vd.grad.cpu().numpy(), f"accumulate C={C}")


@pytest.mark.parametrize("unbounded", [True, False])
def test_contract(hip_lib, oracle, unbounded):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(8)
    aabb = torch.tensor([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0])
    pos = (torch.rand(5000, 3, generator=g) - 0.5) * torch.tensor([400.0, 300.0, 100.0]) + torch.tensor([30.0, 0.0, 10.0])
    pos[0] = torch.tensor([-20.0, 0.0, 5.0])  # on the aabb face -> contracted coordinate outside (0,1) when bounded
    pos[1] = torch.tensor([1e6, -1e6, 3.0])
    ref = oracle.contract(pos, aabb, unbounded)
    dev = _dev()
    pd = pos.to(dev).requires_grad_(True)
    out = ops.contract_points(pd, aabb.to(dev), unbounded)
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), ref.view(np.uint32)), "contraction is bit-exact"
    go = torch.randn(5000, 3, generator=g)
    out.backward(go.to(dev))
    # torch autograd of the reference expression (nerf_utils.py:13-28 + radiance_field.py:294-299), fp64
    p64 = pos.double().requires_grad_(True)
    lo, hi = aabb[:3].double(), aabb[3:].double()
    v = (p64 - lo) / (hi - lo)
    if unbounded:
        v = v * 2 - 1
        mag = torch.linalg.norm(v, ord=float("inf"), dim=-1, keepdim=True)
        v = torch.where(mag < 1, v, (2 - 1 / mag) * (v / mag))
        v = v / 4 + 0.5
    sel = torch.from_numpy((ref != 0).any(-1, keepdims=True)).double()  # selector of the fp32 path
    (v * sel * go.double()).sum().backward()
    ref_g = p64.grad.numpy()
    # held entry by entry to the running-error bound of tests/_bounds.py: the restatement with the fp32 forward's branch decisions
    # is the gradient above (to fp64 rounding) and supplies the intermediates of the bound; the median bound is 0.005 of the
    # earlier rtol = 2e-4 / atol = 1e-6 max|ref| tolerance, and where a cancellation makes it larger the earlier tolerance stays
    dec = UP.model_contract_fwd(pos.numpy(), aabb.numpy(), unbounded)
    assert np.array_equal(dec["out"].view(np.uint32), ref.view(np.uint32))
    st = UP.restate_contract_bwd(pos.numpy(), aabb.numpy(), unbounded, go.numpy(), dec)
    assert np.abs(st["out"] - ref_g).max() <= 1e-12 * np.abs(ref_g).max()
    earlier = 2e-4 * np.abs(ref_g) + 1e-6 * np.abs(ref_g).max()
    assert_err_bound(pd.grad.cpu().numpy(), ref_g, np.minimum(contract_bwd_bounds(st), earlier), f"contract_bwd unbounded={unbounded}")


def test_ray_points(hip_lib, oracle):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(9)
    R, S = 67, 128
    o = torch.rand(R, 3, generator=g) * torch.tensor([60.0, 4.0, 1.0]) + torch.tensor([0.0, -2.0, 1.5])
    d = torch.nn.functional.normalize(torch.tensor([1.0, 0, 0]) + 0.6 * torch.randn(R, 3, generator=g), dim=-1)
    edges = torch.sort(torch.rand(R, S + 1, generator=g) * 300 + 0.1, -1).values
    ts, te = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    aabb = torch.tensor([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0])
    times = torch.rand(R, generator=g)
    pos_ref = (o[:, None, :] + d[:, None, :] * (ts + te)[..., None] / 2.0).numpy()  # render_utils.py:341
    ref = oracle.contract(pos_ref, aabb, True)
    dev = _dev()
    n3, p3 = ops.ray_points(o.to(dev), d.to(dev), ts.to(dev), te.to(dev), aabb.to(dev), True, want_positions=True)
    assert np.array_equal(p3.cpu().numpy().view(np.uint32), pos_ref.view(np.uint32)), "positions are bit-exact"
    assert np.array_equal(n3.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    n4, _ = ops.ray_points(o.to(dev), d.to(dev), ts.to(dev), te.to(dev), aabb.to(dev), True, times=times.to(dev))
    assert np.array_equal(n4[..., :3].cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert torch.equal(n4[..., 3].cpu(), times[:, None].expand(R, S))


def test_dir_encode(hip_lib):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(10)
    d = torch.nn.functional.normalize(torch.randn(1000, 3, generator=g), dim=-1)
    x = (d + 1.0) / 2.0
    scales = torch.tensor([2.0 ** i for i in range(5)])
    xb = (x[..., None, :] * scales[:, None]).reshape(1000, 15)  # encodings.py:95-103
    ref = torch.cat([x, torch.sin(torch.cat([xb, xb + 0.5 * torch.pi], -1))], -1)
    out = ops.dir_encode(d.to(_dev()), 4).cpu()
    assert out.shape == (1000, 33)
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("M,K,N,act,bias", [
    (1000, 32, 64, "relu", True), (257, 64, 64, None, True), (4096, 113, 64, "relu", True),
    (300, 177, 64, "relu", True), (513, 64, 3, "sigmoid", True), (129, 8, 64, "relu", True),
    (777, 64, 1, "trunc_exp", True), (64, 40, 128, None, False), (100, 64, 6, None, True),
    (50, 49, 64, "relu", True), (31, 256, 200, "relu", True),
])
def test_linear(hip_lib, M, K, N, act, bias):
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    dev = _dev()
    xd, Wd = x.to(dev).requires_grad_(True), W.to(dev).requires_grad_(True)
    bd = None if b is None else b.to(dev).requires_grad_(True)
    y = ops.linear(xd, Wd, bd, act)
    x64, W64 = x.double().requires_grad_(True), W.double().requires_grad_(True)
    b64 = None if b is None else b.double().requires_grad_(True)
    pre = torch.nn.functional.linear(x64, W64, b64)
    ref = {None: lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "trunc_exp": lambda t: torch.exp(t - 1)}[act](pre)
    np.testing.assert_allclose(y.detach().cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=2e-6)
    go = torch.randn(M, N, generator=g)
    y.backward(go.to(dev))
    ref.backward(go.double())
    for got, want in ((xd.grad, x64.grad), (Wd.grad, W64.grad)) + (() if b is None else ((bd.grad, b64.grad),)):
        want = want.numpy()
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=2e-5 * np.abs(want).max())


def test_linear_asymmetric_layout(hip_lib):
    """A = I with an asymmetric W catches a transposed MFMA fragment (CDNA guide, G9)."""
    from emernerf_amd import ops
    dev = _dev()
    K, N = 64, 64
    W = (torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 251) / 251.0
    y = ops.linear(torch.eye(K, device=dev), W.to(dev))
    assert torch.equal(y.cpu(), W.t().contiguous())


@pytest.mark.parametrize("n,off", [(100_003, 0), (100_003, 1), (100_000, 3), (5, 2), (2_000_000, 0), (1_234_567, 2)])
def test_adam_matches_torch(hip_lib, n, off):
    """emer_adam_step on a slice that starts ``off`` floats into its buffers (the trainer's groups are views of flat buffers: the
    16-byte vector body of the kernel sits behind a scalar head), any length; elements outside the slice are untouched."""
    from emernerf_amd import ops
    g = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=g)
    ref_p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref_p], lr=0.01, eps=1e-15, weight_decay=1e-5, betas=(0.9, 0.99))  # builders.py:54-60
    dev = _dev()
    pad = 9
    bufs = [torch.full((off + n + pad,), 7.5, device=dev) for _ in range(4)]
    p, gbuf, m, v = (b[off:off + n] for b in bufs)
    p.copy_(p0.to(dev)); m.zero_(); v.zero_()
    for step in range(1, 6):
        grad = torch.randn(n, generator=g) * (0.1 if step != 3 else 0.0)
        ref_p.grad = grad.clone()
        opt.step()
        gbuf.copy_((grad * 1024).to(dev))
        ops.adam_step(p, gbuf, m, v, 0.01, 0.9, 0.99, 1e-15, 1e-5, 1.0 / 1024, step)
    np.testing.assert_allclose(p.cpu().numpy(), ref_p.detach().numpy(), rtol=1e-5, atol=1e-6)
    for b in (bufs[0], bufs[2], bufs[3]):
        assert bool((b[:off] == 7.5).all()) and bool((b[off + n:] == 7.5).all()), "adam_step wrote outside its slice"


def test_cpu_tensor_is_rejected(hip_lib):
    from emernerf_amd import _lib, ops
    with pytest.raises(_lib.EmerError):
        ops.linear(torch.zeros(4, 4), torch.zeros(4, 4))


# ------------------------------------------------------------------------------------- proposal supervision
def _prop_inputs(R, n, m, seed):
    """Final-level edges / transmittance and one proposal level (edges, cdf) shaped like a training step's cache."""
    g = torch.Generator().manual_seed(seed)
    gaps = torch.rand(R, n, generator=g) ** 2 + 1e-4  # strictly increasing edges (a repeated edge is 0/0 in the reference)
    s_fin = torch.cat([torch.zeros(R, 1), torch.cumsum(gaps, -1)], -1)
    s_fin = s_fin / s_fin[:, -1:]
    dens = torch.rand(R, n, generator=g) ** 3 * 40
    dt = s_fin[:, 1:] - s_fin[:, :-1]
    cum = torch.cumsum(dens * dt, -1)
    trans = torch.exp(-torch.cat([torch.zeros(R, 1), cum[:, :-1]], -1))
    s_p = torch.sort(torch.rand(R, m + 1, generator=g), -1).values
    s_p[:, 0], s_p[:, -1] = 0.0, 1.0
    if R > 3:
        s_p[3, 1] = s_p[3, 2]  # a zero-width proposal interval
    w = torch.rand(R, m, generator=g) ** 2 + 1e-4
    c_p = torch.cat([torch.zeros(R, 1), torch.cumsum(w, -1)], -1)
    c_p = c_p / c_p[:, -1:] * (0.6 + 0.4 * torch.rand(R, 1, generator=g))
    return s_fin, trans, s_p, c_p


@pytest.mark.parametrize("R,n,m,level", [(8192, 128, 128, 0), (8192, 128, 64, 1), (37, 48, 64, 0), (5, 16, 16, 1), (3, 200, 300, 1)])
def test_prop_loss_matches_oracle(hip_lib, oracle, R, n, m, level):
    """emer_prop_loss (anti-aliased interlevel loss, value + gradient) vs oracle/ref_path.prop_loss -- the reference's
    formulation with torch.sort and the [R, 2S+2, m] masks (third_party/nerfacc_prop_net.py:22-60,181-238) -- at the
    metric shape R = 8192, S = 128 (oracle evaluated in 512-ray chunks: the loss is a mean over rays)."""
    from emernerf_amd import ops
    from oracle.ref_path import prop_loss
    pulses = (0.03, 0.003)
    s_fin, trans, s_p, c_p = _prop_inputs(R, n, m, seed=R + n + m)
    dev = _dev()
    cd = c_p.to(dev).requires_grad_(True)
    scaler = 1024.0
    loss = ops.prop_level_loss(s_fin.to(dev), trans.to(dev), s_p.to(dev), cd, pulses[level], True, scaler / (R * m))
    (loss * 0.5).backward()  # a non-trivial upstream gradient
    want_loss, want_grad = 0.0, torch.zeros_like(c_p)
    for a in range(0, R, 512):
        b = min(a + 512, R)
        cp = c_p[a:b].clone().requires_grad_(True)
        cache = [(s_p[a:b], cp, level), (s_fin[a:b], None, None)]
        l = prop_loss(cache, trans[a:b], scaler, pulse=pulses) * ((b - a) / R)
        (l * 0.5).backward()
        want_loss += float(l)
        want_grad[a:b] = cp.grad
    assert abs(float(loss) - want_loss) <= 2e-4 * abs(want_loss) + 1e-12
    got = cd.grad.cpu()
    scale = float(want_grad.abs().max())
    err = (got - want_grad).abs()
    # individual entries sit on hinges (max(w_s - w_p, 0)): allow a handful of entries whose hinge flips on rounding
    bad = err > 2e-4 * scale + 2e-3 * want_grad.abs()
    assert int(bad.sum()) <= max(2, got.numel() // 20000), f"{int(bad.sum())} gradient entries off; max err {float(err.max()):.3e} vs scale {scale:.3e}"
    if R <= 64:  # beside the asserts above, at the small shapes (the fp64 mask form is not run at R = 8192): every entry, no exceptions
        from tests._prop_probe import check_total_and_gradient
        check_total_and_gradient(s_fin, trans, s_p, c_p, pulses[level], True, scaler / (R * m), 0.5, float(loss), got.numpy(),
                                 f"prop_loss R={R} n={n} m={m} level {level}")


@pytest.mark.parametrize("R,n,m", [(513, 128, 64), (7, 32, 48)])
def test_pdf_loss_matches_torch_form(hip_lib, R, n, m):
    """emer_prop_loss(anti_aliased=0) vs the reference's _pdf_loss (nerfacc_prop_net.py:342-362) restated in torch with
    nerfacc.searchsorted's bracketing rule."""
    from emernerf_amd import ops
    s_fin, trans, s_p, c_p = _prop_inputs(R, n, m, seed=11 * R + n)
    cdf_q = 1.0 - torch.cat([trans, torch.zeros(R, 1)], -1)
    cp = c_p.clone().requires_grad_(True)
    ir = torch.searchsorted(s_p.contiguous(), s_fin.contiguous(), right=True)
    il = (ir - 1).clamp(0, m)
    ir = ir.clamp(0, m)
    w = cdf_q[:, 1:] - cdf_q[:, :-1]
    w_outer = cp.gather(-1, ir[:, 1:]) - cp.gather(-1, il[:, :-1])
    want = (torch.clip(w - w_outer, min=0) ** 2 / (w + 1e-7)).mean() * 7.0
    want.backward()
    dev = _dev()
    cd = c_p.to(dev).requires_grad_(True)
    got = ops.prop_level_loss(s_fin.to(dev), trans.to(dev), s_p.to(dev), cd, 0.0, False, 7.0 / (R * n))
    got.backward()
    assert abs(float(got) - float(want)) <= 1e-4 * abs(float(want)) + 1e-12
    sc = float(cp.grad.abs().max())
    assert float((cd.grad.cpu() - cp.grad).abs().max()) <= 2e-4 * sc + 1e-12
    if R <= 64:  # beside the asserts above: the per-entry fp64 bound (hit counts and abs-sums of the LDS atomics)
        from tests._prop_probe import check_total_and_gradient
        check_total_and_gradient(s_fin, trans, s_p, c_p, 0.0, False, 7.0 / (R * n), 1.0, float(got), cd.grad.cpu().numpy(), f"pdf_loss R={R} n={n} m={m}")


# ----------------------------------------------------------------------------- per-ray epilogue and pixel losses
@pytest.mark.parametrize("R,with_sky", [(1, True), (1000, True), (8192, False)])
def test_ray_epilogue_matches_torch(hip_lib, R, with_sky):
    """emer_ray_epilogue_* vs the reference's per-ray torch chain (render_utils.py:102-105,217-220) in fp64, values and
    gradients, including rays whose sum of weights sits outside the clamp range."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R)
    stats = torch.rand(R, 4, generator=g)
    stats[:, 1] *= 30
    if R > 10:
        stats[1, 0] = 1.0 + 3e-7   # above the clamp: gradient of the sum is cut
        stats[2, 0] = 1e-8         # below
        stats[3, 0] = 1.0          # on the bound: passes (torch convention)
    acc = torch.rand(R, 3, generator=g)
    sky = torch.rand(R, 3, generator=g) if with_sky else None
    sd, ad = stats.to(dev).requires_grad_(True), acc.to(dev).requires_grad_(True)
    kd = None if sky is None else sky.to(dev).requires_grad_(True)
    opa, dep, med, rgb = ops.ray_epilogue(sd, ad, kd)
    go, gd, gr = torch.randn(R, 1, generator=g), torch.randn(R, 1, generator=g), torch.randn(R, 3, generator=g)
    ((opa * go.to(dev)).sum() + (dep * gd.to(dev)).sum() + (rgb * gr.to(dev)).sum()).backward()
    s64, a64 = stats.double().requires_grad_(True), acc.double().requires_grad_(True)
    k64 = None if sky is None else sky.double().requires_grad_(True)
    o = s64[:, 0:1].clamp(float(np.float32(1e-6)), 1.0)
    d = s64[:, 1:2] / o
    c = a64 if k64 is None else a64 + k64 * (1.0 - o)
    ((o * go.double()).sum() + (d * gd.double()).sum() + (c * gr.double()).sum()).backward()
    np.testing.assert_allclose(opa.detach().cpu().numpy(), o.detach().numpy(), rtol=1e-6)
    np.testing.assert_allclose(dep.detach().cpu().numpy(), d.detach().numpy(), rtol=2e-6)
    np.testing.assert_allclose(rgb.detach().cpu().numpy(), c.detach().numpy(), rtol=2e-6, atol=1e-7)
    assert torch.equal(med.cpu()[:, 0], stats[:, 2])
    gs = sd.grad.cpu().double()
    assert float(gs[:, 2:].abs().max()) == 0.0
    np.testing.assert_allclose(gs[:, :2].numpy(), s64.grad[:, :2].numpy(), rtol=1e-4, atol=1e-5 * float(s64.grad.abs().max()))
    np.testing.assert_allclose(ad.grad.cpu().numpy(), a64.grad.numpy(), rtol=1e-6)
    if sky is not None:
        np.testing.assert_allclose(kd.grad.cpu().numpy(), k64.grad.numpy(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("R", [1, 777, 8192])
def test_pixel_loss_matches_torch(hip_lib, R):
    """emer_pixel_loss_* vs F.mse_loss + 0.001 * F.binary_cross_entropy (loss/base.py:83-185 as the trainer applies
    them), incl. opacities of exactly 1 and 1e-6 (torch clamps the logs at -100)."""
    import torch.nn.functional as Fn
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R + 5)
    rgb, pix = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    opa = torch.rand(R, 1, generator=g).clamp(1e-6, 1.0)
    sky = (torch.rand(R, generator=g) < 0.3).float()
    if R > 4:
        opa[0], opa[1], opa[2], opa[3] = 1.0, 1.0, 1e-6, 1e-6
        sky[0], sky[1], sky[2], sky[3] = 1.0, 0.0, 1.0, 0.0
    rd, od = rgb.to(dev).requires_grad_(True), opa.to(dev).requires_grad_(True)
    loss = ops.pixel_loss(rd, od, pix.to(dev), sky.to(dev), 1.0, 0.001)
    (loss * 1024.0).backward()
    r2, o2 = rgb.clone().requires_grad_(True), opa.clone().requires_grad_(True)
    want = Fn.mse_loss(r2.squeeze(), pix.squeeze()) + 0.001 * Fn.binary_cross_entropy(o2.squeeze(-1), 1 - sky)
    (want * 1024.0).backward()
    np.testing.assert_allclose(float(loss), float(want), rtol=2e-6)
    np.testing.assert_allclose(rd.grad.cpu().numpy(), r2.grad.numpy(), rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(od.grad.cpu().numpy(), o2.grad.numpy(), rtol=1e-5, atol=1e-9)
    if R <= 777:   # every gradient entry inside its first-order fp64 bound (tests/_bounds.pixel_bounds), the total inside the sum of the per-ray bounds
        from tests import _loss_probe as LP
        from tests._bounds import U, assert_err_bound, pixel_bounds
        st = LP.restate_pixel(rgb.numpy(), pix.numpy(), opa.numpy().reshape(-1), sky.numpy(), 1.0, 0.001, up=1024.0)
        bd = pixel_bounds(st)
        assert_err_bound(rd.grad.cpu().numpy(), st["d_rgb"], bd["d_rgb"], f"pixel_loss R={R} d_rgb")
        assert_err_bound(od.grad.cpu().numpy(), st["d_opa"], bd["d_opa"], f"pixel_loss R={R} d_opacity")
        assert abs(float(loss) - st["total"]) <= bd["rays"].sum() + U * abs(st["total"])


@pytest.mark.parametrize("R,S,E,terms", [(64, 16, 8, "dsfc"), (8192, 128, 64, "dsfc"), (777, 33, 5, "dc"), (1000, 64, 64, "f"),
                                          (3, 1, 1, "ds"), (4096, 128, 64, "c")])
def test_reg_losses_match_the_reference_expressions(hip_lib, R, S, E, terms):
    """emer_reg_losses_fwd/bwd (row N4) vs the reference's own expressions evaluated by torch in fp64: dynamic-density and
    shadow sparsity ``coef * x.mean()`` (loss/base.py:394-398 with default_config.yaml's 0.01), feature L2 ``0.5 * mse``
    (loss/base.py:83-146), flow cycle ``0.01 * 0.5 * ((ff.detach() + fpb) ** 2 + (bf.detach() + bpf) ** 2).mean()``
    (train_emernerf.py:700-716), added to a base scalar; gradients scaled by the trainer's loss scale; the detached flows get none."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R * 7 + S)
    base = torch.rand((), generator=g)
    dyn, sh = torch.rand(R, S, generator=g) * 3, torch.rand(R, 1, generator=g)
    ft, gt = torch.randn(R, E, generator=g), torch.rand(R, E, generator=g)
    ff, fpb, bf, bpf = (torch.randn(R, S, 3, generator=g) * 0.3 for _ in range(4))
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in dict(base=base, dyn=dyn, sh=sh, ft=ft, ff=ff, fpb=fpb, bf=bf, bpf=bpf).items()}
    kw = {}
    if "d" in terms:
        kw["dynamic_density"] = leaves["dyn"]
    if "s" in terms:
        kw["shadow_ratio"] = leaves["sh"]
    if "f" in terms:
        kw.update(feat=leaves["ft"], feat_gt=gt.to(dev))
    if "c" in terms:
        kw.update(forward_flow=leaves["ff"], forward_pred_backward_flow=leaves["fpb"], backward_flow=leaves["bf"],
                  backward_pred_forward_flow=leaves["bpf"])
    scale = 1024.0
    out = ops.reg_losses(leaves["base"], grad_scale=scale, **kw)
    out.backward()
    ref = {k: v.double().clone().requires_grad_(True) for k, v in dict(base=base, dyn=dyn, sh=sh, ft=ft, ff=ff, fpb=fpb, bf=bf, bpf=bpf).items()}
    reg = torch.zeros((), dtype=torch.float64)
    if "d" in terms:
        reg = reg + 0.01 * ref["dyn"].mean()
    if "s" in terms:
        reg = reg + 0.01 * ref["sh"].mean()
    if "f" in terms:
        reg = reg + 0.5 * torch.nn.functional.mse_loss(ref["ft"], gt.double())
    if "c" in terms:
        reg = reg + 0.01 * 0.5 * ((ref["ff"].detach() + ref["fpb"]) ** 2 + (ref["bf"].detach() + ref["bpf"]) ** 2).mean()
    (ref["base"] + reg * scale).backward()   # the base passes its gradient through unscaled (its own kernel folded the scale)
    np.testing.assert_allclose(float(out), float(ref["base"] + reg), rtol=3e-6)
    used = {"base"} | ({"dyn"} if "d" in terms else set()) | ({"sh"} if "s" in terms else set()) | ({"ft"} if "f" in terms else set()) \
        | ({"fpb", "bpf"} if "c" in terms else set())
    for k, leaf in leaves.items():
        if k in used:
            np.testing.assert_allclose(leaf.grad.cpu().numpy(), ref[k].grad.numpy(), rtol=2e-6, atol=1e-12, err_msg=k)
        else:
            assert leaf.grad is None, f"{k} must not receive a gradient"
    # run-to-run bit-stable (fixed summation order)
    again = ops.reg_losses(leaves["base"].detach(), grad_scale=scale, **{k: v.detach() for k, v in kw.items()})
    assert torch.equal(again, out.detach())
    if R <= 777:   # every gradient entry within its few roundings of fp64, the total inside the sum of the block partials' abs-sum bounds
        from tests import _loss_probe as LP
        from tests._bounds import U
        T = {}
        if "d" in terms:
            T["dyn"] = dyn.numpy()
        if "s" in terms:
            T["shadow"] = sh.numpy()
        if "f" in terms:
            T.update(feat=ft.numpy(), feat_gt=gt.numpy())
        if "c" in terms:
            T.update(ff=ff.numpy(), fpb=fpb.numpy(), bf=bf.numpy(), bpf=bpf.numpy())
        b = dict(T=T, coefs=dict(dyn=0.01, shadow=0.01, feat=0.5, cycle=0.005), base=float(base), up=1.0, grad_scale=scale)
        b["ref"] = LP.restate_reg(T, b["coefs"], b["base"], 1.0, scale)
        got = {n: leaves[k].grad.cpu().numpy() for n, k in (("dyn", "dyn"), ("shadow", "sh"), ("feat", "ft"), ("fpb", "fpb"), ("bpf", "bpf")) if k in used}
        LP.check_reg_realistic(b, None, float(out), got, f"reg_losses R={R} S={S} E={E} {terms}")
        err = LP.reg_block_refs(b)[1]
        assert abs(float(out) - b["ref"]["total"]) <= err.sum() + U * abs(b["ref"]["total"])


@pytest.mark.parametrize("R,m,n,unbounded,want_pos,jit", [(8192, 129, 64, True, False, True), (100, 2, 128, True, True, True),
                                                          (1031, 65, 128, False, True, False), (7, 33, 1, True, False, True),
                                                          (513, 129, 128, True, True, True)])
def test_importance_sample_points_equals_the_two_launches(hip_lib, R, m, n, unbounded, want_pos, jit):
    """ops.importance_sample(points=...) -- the sampler and, in the same launch, the sample points of the intervals it produced -- gives
    BITWISE the edges / interval starts / ends of emer_importance_sample and the contracted points (and world positions) emer_ray_points
    computes from them (same device functions and expression order, FMA contraction off in both translation units): the sample positions
    decide the grid cells, so nothing less than bit equality will do."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R + m + n)
    vals = torch.sort(torch.rand(R, m, generator=g), dim=-1).values
    vals[:, 0], vals[:, -1] = 0.0, 1.0
    w = torch.rand(R, m - 1, generator=g) + 1e-3
    w[R // 3] = 0.0
    w[R // 3, 0] = 1.0   # a ray whose mass sits in one bin
    cdfs = torch.cat([torch.zeros(R, 1), torch.cumsum(w / w.sum(-1, keepdim=True), -1)], -1)
    jitter = torch.rand(R, generator=g).to(dev) if jit else None
    o = (torch.rand(R, 3, generator=g) * 60 - 10).to(dev)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
    aabb = torch.tensor([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0]).to(dev)
    planes = (0.1, 1000.0, "uniform_lindisp")
    e0, a0, b0 = ops.importance_sample(vals.to(dev), cdfs.to(dev), n, jitter, stot=planes, intervals=True)
    n0, p0 = ops.ray_points(o, d, a0, b0, aabb, unbounded, want_positions=want_pos)
    e1, a1, b1, n1, p1 = ops.importance_sample(vals.to(dev), cdfs.to(dev), n, jitter, stot=planes, intervals=True,
                                              points=(o, d, aabb, unbounded, want_pos))
    for name, x, y in (("edges", e0, e1), ("starts", a0, a1), ("ends", b0, b1), ("normed", n0, n1)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
    assert (p1 is None) == (not want_pos)
    if want_pos:
        assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


@pytest.mark.parametrize("R,S,terms", [(64, 16, "dsc"), (333, 7, "c"), (2048, 128, "dc")])
def test_reg_losses_flow_pair_equals_the_four_slices(hip_lib, R, S, terms):
    """ops.reg_losses(flow_pair=(flow [R,S,6], flow2 [2 R S, 6])) -- the cycle term read from the flow MLP's own outputs
    (emer_reg_losses_fwd6 / bwd6) -- gives BITWISE the loss of the four-slice form (same summation order) and the same gradient,
    delivered as one [2 N, 6] tensor with zeros in the column blocks the loss does not read; the flow at the samples gets none."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R + S)
    N = R * S
    base = torch.rand((), generator=g).to(dev)
    dyn, sh = (torch.rand(R, S, generator=g) * 3).to(dev), torch.rand(R, 1, generator=g).to(dev)
    flow = (torch.randn(R, S, 6, generator=g) * 0.3).to(dev).requires_grad_(True)
    flow2 = (torch.randn(2 * N, 6, generator=g) * 0.3).to(dev).requires_grad_(True)
    kw = {}
    if "d" in terms:
        kw["dynamic_density"] = dyn
    if "s" in terms:
        kw["shadow_ratio"] = sh
    out = ops.reg_losses(base, grad_scale=1024.0, flow_pair=(flow, flow2), **kw)
    out.backward()
    f_ref, f2_ref = flow.detach().clone().requires_grad_(True), flow2.detach().clone().requires_grad_(True)
    fwd_pred, bwd_pred = (t.view(R, S, 6) for t in f2_ref.split(N, dim=0))
    want = ops.reg_losses(base, grad_scale=1024.0, forward_flow=f_ref[..., :3], backward_flow=f_ref[..., 3:],
                          forward_pred_backward_flow=fwd_pred[..., 3:], backward_pred_forward_flow=bwd_pred[..., :3], **kw)
    want.backward()
    assert torch.equal(out.detach(), want.detach()), "same terms in the same order: the loss must be bitwise the sliced form's"
    assert flow.grad is None and f_ref.grad is None
    assert torch.equal(flow2.grad, f2_ref.grad)
    assert float(flow2.grad[:N, :3].abs().max()) == 0.0 and float(flow2.grad[N:, 3:].abs().max()) == 0.0
    if R <= 777:   # the packed form held directly to fp64, not only to the sliced form
        from tests import _loss_probe as LP
        from tests._bounds import U
        T = dict(flow6=flow.detach().cpu().numpy().reshape(-1, 6), flow2=flow2.detach().cpu().numpy())
        if "d" in terms:
            T["dyn"] = dyn.cpu().numpy()
        if "s" in terms:
            T["shadow"] = sh.cpu().numpy()
        b = dict(T=T, coefs=dict(dyn=0.01, shadow=0.01, feat=0.5, cycle=0.005), base=float(base), up=1.0, grad_scale=1024.0)
        b["ref"] = LP.restate_reg(T, b["coefs"], b["base"], 1.0, 1024.0)
        LP.check_reg_realistic(b, None, float(out), dict(flow2=flow2.grad.cpu().numpy()), f"reg_losses flow_pair R={R} S={S} {terms}")
        err = LP.reg_block_refs(b)[1]
        assert abs(float(out) - b["ref"]["total"]) <= err.sum() + U * abs(b["ref"]["total"])


def test_reg_losses_argument_errors(hip_lib):
    from emernerf_amd import _lib, ops
    dev = _dev()
    with pytest.raises(ValueError):
        ops.reg_losses()
    with pytest.raises(AssertionError):
        ops.reg_losses(None, feat=torch.zeros(4, 3, device=dev), feat_gt=torch.zeros(4, 2, device=dev))
    with pytest.raises(_lib.EmerError):
        ops.reg_losses(None, dynamic_density=torch.zeros(4, 3))   # CPU tensor: there is no fallback
    assert float(ops.reg_losses(torch.full((), 2.5, device=dev))) == 2.5   # no term present: the base itself


@pytest.mark.parametrize("N,unbounded", [(5000, True), (37, True), (4096, False)])
def test_flow_warp_matches_the_torch_chain(hip_lib, N, unbounded):
    """emer_flow_warp_fwd/bwd vs the reference's expressions (radiance_field.py:567-580) evaluated op by op on the HIP contraction:
    ``contract(positions + flow * noise)``, ``clamp(t +- time_diff * noise, 0, 1)`` and the batch assembly -- forward BIT-exact, the
    gradient w.r.t. the flow equal to autograd's through the same chain (fp32, 1e-6 relative)."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(N)
    aabb = torch.tensor([-20.0, -40.0, 0.0, 80.0, 40.0, 20.0]).to(dev)
    pos = (torch.rand(N, 3, generator=g) * torch.tensor([300.0, 200.0, 60.0]) - torch.tensor([100.0, 100.0, 20.0])).to(dev)   # inside and far outside the box
    normed = ops.contract_points(pos, aabb, unbounded)
    ts = (torch.randint(0, 10, (N, 1), generator=g).float() / 9).to(dev)
    flow = (torch.randn(N, 6, generator=g) * 2.0).to(dev).requires_grad_(True)
    noise = torch.rand(N, 1, generator=g).to(dev)
    dt = 0.1
    x3, x2 = ops.flow_warp(pos, normed, ts, flow, noise, dt, aabb, unbounded)
    f2 = flow.detach().clone().requires_grad_(True)
    fwd_pos = ops.contract_points(pos + f2[:, :3] * noise, aabb, unbounded)
    bwd_pos = ops.contract_points(pos + f2[:, 3:] * noise, aabb, unbounded)
    x_fwd = torch.cat([fwd_pos, torch.clamp(ts + dt * noise, 0, 1.0)], -1)
    x_bwd = torch.cat([bwd_pos, torch.clamp(ts - dt * noise, 0, 1.0)], -1)
    want3 = torch.cat([torch.cat([normed, ts], -1), x_fwd, x_bwd], 0)
    assert torch.equal(x3.detach(), want3.detach()) and torch.equal(x2.detach(), want3.detach()[N:])
    g3, g2 = torch.randn(3 * N, 4, generator=g).to(dev), torch.randn(2 * N, 4, generator=g).to(dev)
    ((x3 * g3).sum() + (x2 * g2).sum()).backward()
    ((want3 * g3).sum() + (want3[N:] * g2).sum()).backward()
    np.testing.assert_allclose(flow.grad.cpu().numpy(), f2.grad.cpu().numpy(), rtol=2e-6, atol=1e-9)
    # one consumer only (the other output unused): the missing gradient is a structural zero
    flow.grad = None
    x3b, _ = ops.flow_warp(pos, normed, ts, flow, noise, dt, aabb, unbounded)
    (x3b * g3).sum().backward()
    f2.grad = None
    fwd_pos = ops.contract_points(pos + f2[:, :3] * noise, aabb, unbounded)
    bwd_pos = ops.contract_points(pos + f2[:, 3:] * noise, aabb, unbounded)
    (torch.cat([fwd_pos, bwd_pos], 0) * g3[N:, :3]).sum().backward()
    np.testing.assert_allclose(flow.grad.cpu().numpy(), f2.grad.cpu().numpy(), rtol=2e-6, atol=1e-9)


# ------------------------------------------------------------------------------------ training-ray generation
def _ref_get_rays(x, y, c2w, K):
    """datasets/base/pixel_source.py:39-76 restated (the reference module cannot travel to the GPU box)."""
    cam = torch.nn.functional.pad(torch.stack([(x - K[:, 0, 2] + 0.5) / K[:, 0, 0], (y - K[:, 1, 2] + 0.5) / K[:, 1, 1]], -1), (0, 1), value=1.0)
    d = (cam[:, None, :] * c2w[:, :3, :3]).sum(-1)
    o = torch.broadcast_to(c2w[:, :3, -1], d.shape)
    n = torch.linalg.norm(d, dim=-1, keepdims=True)
    return o, d / (n + 1e-8), n


def test_gen_rays_and_train_batch(hip_lib):
    """emer_gen_rays vs get_rays + the index gathers of get_train_rays (pixel_source.py:670-731); uniform sampling ranges."""
    from emernerf_amd.pixel_source import PixelSource, get_rays
    dev = _dev()
    src = PixelSource.synthetic(dev, num_imgs=12, height=48, width=64, num_cams=3, seed=4)
    batch = src.get_train_rays(5000, candidate_indices=[1, 4, 7, 10])
    img, pc = batch["img_idx"].cpu(), batch["pixel_coords"].cpu()
    assert set(img.tolist()) <= {1, 4, 7, 10} and len(set(img.tolist())) == 4
    y, x = (pc[:, 0] * 48).round().long(), (pc[:, 1] * 64).round().long()
    assert int(y.min()) == 0 and int(y.max()) == 47 and int(x.min()) == 0 and int(x.max()) == 63
    o, d, n = _ref_get_rays(x.float(), y.float(), src.cam_to_worlds.cpu()[img], src.intrinsics.cpu()[img])
    np.testing.assert_allclose(batch["origins"].cpu().numpy(), o.numpy(), rtol=0, atol=0)
    np.testing.assert_allclose(batch["viewdirs"].cpu().numpy(), d.numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(batch["direction_norms"].cpu().numpy(), n.numpy(), rtol=2e-7)
    assert torch.equal(batch["pixels"].cpu(), src.images.cpu()[img, y, x])
    assert torch.equal(batch["sky_masks"].cpu(), src.sky_masks.cpu()[img, y, x])
    assert torch.equal(batch["normed_timestamps"].cpu(), src.normalized_timestamps.cpu()[img])
    assert torch.equal(batch["cam_idx"].cpu(), src.cam_ids.cpu()[img])
    # a new batch differs (the seed word advances on the device), and the stand-alone get_rays agrees
    b2 = src.get_train_rays(5000, candidate_indices=[1, 4, 7, 10])
    assert not torch.equal(b2["pixel_coords"], batch["pixel_coords"])
    o2, d2, n2 = get_rays(x.to(dev), y.to(dev), src.cam_to_worlds[img.to(dev)], src.intrinsics[img.to(dev)])
    assert torch.equal(o2, batch["origins"]) and torch.equal(d2, batch["viewdirs"])
    # render rays: every pixel of image 5, image-shaped
    rr = src.get_render_rays(5)
    assert rr["origins"].shape == (48, 64, 3) and rr["pixels"].shape == (48, 64, 3) and rr["sky_masks"].shape == (48, 64)
    assert torch.equal(rr["pixels"], src.images[5])


def test_importance_sampling_without_replacement(hip_lib):
    """emer_sample_importance == torch.multinomial(w, k, replacement=False) in distribution: k distinct indices, never a
    zero-weight one, inclusion frequencies within 5 sigma of torch's own over 3000 draws; and a million-entry buffer."""
    import ctypes
    from emernerf_amd import _lib, ops
    dev = _dev()
    g = torch.Generator().manual_seed(0)
    n, k, draws = 64, 8, 3000
    w = torch.rand(n, generator=g) ** 3
    w[5], w[17] = 0.0, 0.0
    wd = w.to(dev)
    ws = torch.empty(4 + 2048, dtype=torch.int32, device=dev)
    out = torch.empty(k, dtype=torch.int64, device=dev)
    counts = torch.zeros(n)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in range(draws):
        seed.fill_(t * 7919 + 1)
        _lib.call("emer_sample_importance", ops._ptr(wd), n, ops._ptr(seed), 0, k, ops._ptr(ws), ops._ptr(out), ops._stream(wd))
        o = out.cpu()
        assert len(set(o.tolist())) == k and int(o.min()) >= 0 and int(o.max()) < n
        counts[o] += 1
    assert counts[5] == 0 and counts[17] == 0
    ref = torch.zeros(n)
    gg = torch.Generator().manual_seed(1)
    for _ in range(draws):
        ref[torch.multinomial(w, k, replacement=False, generator=gg)] += 1
    p = ref / draws
    sigma = torch.sqrt(p * (1 - p) / draws).clamp_min(1e-3) * (2 ** 0.5)
    assert float(((counts / draws - p).abs() / sigma).max()) < 5.0
    # error-buffer scale: 200 images at 160 x 240 -> 7.68 M weights, 2048 winners
    big = torch.rand(200 * 160 * 240, generator=g).to(dev)
    big[::3] = 0.0
    o = torch.empty(2048, dtype=torch.int64, device=dev)
    _lib.call("emer_sample_importance", ops._ptr(big), big.numel(), ops._ptr(seed), 5, 2048, ops._ptr(ws), ops._ptr(o), ops._stream(big))
    oc = o.cpu()
    assert len(set(oc.tolist())) == 2048 and float(big[o].min()) > 0.0
    assert float(big[o].mean()) > 0.6  # weights ~U(0,1): winners are biased to heavy entries (E[w | picked] = 2/3)
    # through the PixelSource API
    from emernerf_amd.pixel_source import PixelSource
    src = PixelSource.synthetic(dev, num_imgs=6, height=32, width=48, seed=2, buffer_ratio=0.2)
    src.build_pixel_error_buffer()
    err = torch.zeros(6, 8, 12)
    err[2, 3, 4] = 1.0
    err[4] = 0.5
    src.update_pixel_error_maps(torch.zeros(6, 8, 12, 3), err[..., None].expand(-1, -1, -1, 3))
    b = src.get_train_rays(400)
    assert b["origins"].shape == (400, 3)
    roi = b["img_idx"].cpu()[320:]  # the last fifth (80 rays) comes from the buffer: only images 2 and 4 (97 cells) carry error
    assert set(roi.tolist()) <= {2, 4}
    # the public sampling methods draw fresh pixels on every call (the seed only advanced in get_train_rays) ...
    u1, u2 = src.sample_uniform_rays(256), src.sample_uniform_rays(256)
    assert not all(torch.equal(a, b_) for a, b_ in zip(u1, u2))
    i1, i2 = src.sample_important_rays(40), src.sample_important_rays(40)
    assert not all(torch.equal(a, b_) for a, b_ in zip(i1, i2))
    # ... and, like torch.multinomial, refuse to draw more cells without replacement than carry weight (97 here)
    with pytest.raises(RuntimeError, match="positive weight"):
        src.sample_important_rays(98)


# ---------------------------------------------------------------------------------------------- lidar losses
@pytest.mark.parametrize("R,S", [(1, 16), (300, 64), (4096, 128)])
def test_lidar_loss_matches_reference_form(hip_lib, R, S):
    """emer_lidar_loss vs the reference's DepthLoss("l2") + compute_line_of_sight_loss (loss/base.py:188-271,430-464)
    restated literally in torch fp64 (including the scalar-mean x per-ray-mask product), values and gradients."""
    import math
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R + S)
    t = torch.sort(torch.rand(R, S, generator=g) * 90, -1).values
    w = torch.rand(R, S, generator=g) ** 2 * 0.1
    gt = torch.rand(R, 1, generator=g) * 100 - 5  # some <= 0, some beyond 80 m
    depth = torch.rand(R, 1, generator=g) * 100 - 5
    eps, coef = 3.7, 0.05
    dd, wd = depth.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    loss = ops.lidar_loss(dd, wd, gt.to(dev), t.to(dev), eps, 80.0, 1.0, coef)
    (loss * 3.0).backward()

    d64, w64 = depth.double().requires_grad_(True), w.double().requires_grad_(True)
    g64, t64 = gt.double().squeeze(-1), t.double()
    # the masks are integer facts: taken from the fp32 comparisons the reference itself performs (fp32 tensors against fl32(gt -+ eps))
    valid = (gt.squeeze(-1) > 0.01) & (gt.squeeze(-1) < 80.0)
    norm = lambda v: torch.clamp(v / 80.0, 0.0, 1.0)  # noqa: E731
    depth_loss = ((norm(d64.squeeze(-1)[valid]) - norm(g64[valid])) ** 2).mean() if bool(valid.any()) else torch.zeros((), dtype=torch.float64)
    gd = g64.unsqueeze(-1)
    empty = t < gt - eps
    near = (t > (gt - eps)) & (t < gt + eps)
    sigma = eps / 3
    delta = (1 / math.sqrt(2 * math.pi * sigma ** 2)) * torch.exp(-((t64 - gd) ** 2) / (2 * sigma ** 2))
    empty_loss = (w64.square() * empty).sum(-1, keepdim=True).mean()
    near_loss = ((w64 - delta).square() * near).sum(-1, keepdim=True).mean()
    sight = ((empty_loss + near_loss) * (gt.squeeze(-1) > 0)).mean() * coef
    want = depth_loss + sight
    (want * 3.0).backward()
    np.testing.assert_allclose(float(loss), float(want), rtol=2e-5)
    np.testing.assert_allclose(dd.grad.cpu().numpy(), d64.grad.numpy(), rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(wd.grad.cpu().numpy(), w64.grad.numpy(), rtol=1e-4, atol=1e-7 * float(w64.grad.abs().max()))
    if R <= 777:   # every gradient entry inside its first-order fp64 bound (tests/_bounds.lidar_bounds), the total inside the sum of the per-ray bounds
        from tests import _loss_probe as LP
        from tests._bounds import U, assert_err_bound, lidar_bounds
        st = LP.restate_lidar(depth.numpy(), gt.numpy(), w.numpy(), t.numpy(), eps, 80.0, 1.0, coef, up=3.0)
        if st["n_valid"]:
            np.testing.assert_allclose(st["total_ref"], float(want), rtol=1e-12)
        bd = lidar_bounds(st, eps)
        assert_err_bound(dd.grad.cpu().numpy(), st["d_depth"], bd["d_depth"], f"lidar_loss R={R} S={S} d_depth")
        assert_err_bound(wd.grad.cpu().numpy(), st["d_w"], bd["d_w"], f"lidar_loss R={R} S={S} d_weights")
        assert abs(float(loss) - st["total"]) <= bd["rays"].sum() + U * abs(st["total"])


@pytest.mark.parametrize("R,S,with_shadow", [(3, 16, True), (257, 128, True), (100, 70, False)])
def test_blend_accumulate_matches_torch(hip_lib, R, S, with_shadow):
    """emer_blend_accumulate_* vs the reference's static / dynamic / shadow blend (render_utils.py:125-175) in fp64."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(R * S)
    rnd = lambda *sh: torch.rand(*sh, generator=g)  # noqa: E731
    w, ss, sd = rnd(R, S) * 0.1, rnd(R, S) * 3, rnd(R, S) * 2
    ss[0, 0] = sd[0, 0] = 0.0  # empty sample: ratios 0 / 1e-6
    rs, rd, sh = rnd(R, S, 3), rnd(R, S, 3), rnd(R, S, 1)
    names = ["w", "ss", "sd", "rs", "rd"] + (["sh"] if with_shadow else [])
    cpu = {"w": w, "ss": ss, "sd": sd, "rs": rs, "rd": rd, "sh": sh}
    dv = {k: cpu[k].to(dev).requires_grad_(True) for k in names}
    sig = dv["ss"] + dv["sd"]
    acc, acs = ops.blend_accumulate(dv["w"], sig, dv["ss"], dv["sd"], dv["rs"], dv["rd"], dv.get("sh"))
    g_rgb, g_sh = torch.randn(R, 3, generator=g), torch.randn(R, 1, generator=g)
    loss = (acc * g_rgb.to(dev)).sum()
    if with_shadow:
        loss = loss + (acs * g_sh.to(dev)).sum()
    loss.backward()
    d64 = {k: cpu[k].double().requires_grad_(True) for k in names}
    s64 = d64["ss"] + d64["sd"]
    a, b = d64["ss"] / (s64 + 1e-6), d64["sd"] / (s64 + 1e-6)
    shd = d64["sh"] if with_shadow else 0.0
    rgb = a[..., None] * d64["rs"] * (1 - shd) + b[..., None] * d64["rd"]
    want = (d64["w"][..., None] * rgb).sum(1)
    l64 = (want * g_rgb.double()).sum()
    if with_shadow:
        want_s = (d64["w"][..., None] * d64["sh"].square()).sum(1)
        l64 = l64 + (want_s * g_sh.double()).sum()
        np.testing.assert_allclose(acs.detach().cpu().numpy(), want_s.detach().numpy(), rtol=2e-5, atol=1e-7)
    l64.backward()
    np.testing.assert_allclose(acc.detach().cpu().numpy(), want.detach().numpy(), rtol=2e-5, atol=1e-7)
    for k in names:
        ref_g = d64[k].grad
        np.testing.assert_allclose(dv[k].grad.cpu().numpy(), ref_g.numpy(), rtol=1e-4, atol=2e-6 * float(ref_g.abs().max()), err_msg=k)
    # per entry (tests/_bounds.py blend_c); sigma_s and sigma_d also carry the gradient of the device sum sigma
    if R <= 257:
        p = dict(w=w.numpy(), sig=sig.detach().cpu().numpy(), ss=ss.numpy(), sd=sd.numpy(), rs=rs.numpy(), rd=rd.numpy(),
                 sh=sh.numpy()[..., 0] if with_shadow else None, g_rgb=g_rgb.numpy(), g_sh=g_sh.numpy() if with_shadow else None)
        got = {"d_" + k: dv[k].grad.cpu().numpy().reshape(cpu[k].shape[:3] if cpu[k].shape[-1] == 3 else (R, S)) for k in names}
        got.update(acc=acc.detach().cpu().numpy(), acs=acs.detach().cpu().numpy()[:, 0] if with_shadow else None)
        CP.check_real_blend_through_sum(p, got, f"blend R={R} S={S}")


def test_nonfinite_gradient_is_reported_before_the_scatter(hip_lib, oracle, monkeypatch):
    """DESIGN 4.1 "Determinism and numerics": the run reduction of the owner-computes backward multiplies neighbours by 0/1 masks,
    so one inf in the incoming gradient turns OTHER table entries of its wave into NaN (upstream's atomics keep it local).  That
    behaviour is pinned here, and so is the debug check (EMER_CHECK_FINITE=1 / ops.CHECK_FINITE) that names the offending
    (level, sample) before the scatter -- the table gradient alone would point at the wrong entries."""
    from emernerf_amd import _lib, ops
    monkeypatch.setattr(ops, "CHECK_FINITE", False)  # (the suite may be run with EMER_CHECK_FINITE=1)
    meta = oracle.grid_meta_from_encoder_args(3, 16, 16, 2048, 19, 2)
    desc = _lib.make_grid_desc(3, 16, 2, 19, 16, meta.per_level_scale)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    N = 4096
    x = torch.rand(N, 3, generator=g).to(dev)
    p = (torch.rand(meta.n_params, generator=g) - 0.5).to(dev).requires_grad_(True)
    dlm = torch.randn(16, N, 2, generator=g).to(dev)
    clean = dlm.clone()
    dlm[5, 1234, 1] = float("inf")
    lm = ops.hashgrid_encode_lm(x, p, desc)
    lm.backward(dlm)
    bad = ~torch.isfinite(p.grad)
    lo, hi = int(meta.offset[5]) * 2, (int(meta.offset[5]) + int(meta.size[5])) * 2
    assert bool(bad.any()) and not bool(bad[:lo].any()) and not bool(bad[hi:].any()), "contamination must stay inside the level"
    p.grad = None
    monkeypatch.setattr(ops, "CHECK_FINITE", True)
    lm = ops.hashgrid_encode_lm(x, p, desc)
    with pytest.raises(FloatingPointError, match=r"\[5, 1234\]"):
        lm.backward(dlm)
    lm = ops.hashgrid_encode_lm(x, p, desc)
    lm.backward(clean)   # finite gradients pass the check
    assert bool(torch.isfinite(p.grad).all())


# ------------------------------------------------------------------------------------------ per-ray inputs of the heads
@pytest.mark.parametrize("R,n_emb,E,max_deg", [(8192, 150, 16, 4), (8192, 2, 16, 4), (37, 3, 16, 4), (513, 1000, 5, 2), (64, 1, 16, 0), (5000, 1, 20, 4)])
def test_ray_inputs_and_embedding_gradient(hip_lib, R, n_emb, E, max_deg):
    """emer_ray_inputs_fwd == [emer_dir_encode | weight[idx]] bit for bit (rgb rows on remapped directions, sky rows on raw
    ones); emer_embed_grad == index_add of the two consumers' gradients in fp64 (tolerance 1e-6 relative to the largest
    entry: fp32 sums of up to R terms) and per entry within c_embed_grad(R) u sum |g| (tests/_bounds.py), and is deterministic
    (two runs bit-identical).  Bit for bit on exact probes: tests/test_ray_exact_gpu.py."""
    from emernerf_amd import fused, ops
    dev = _dev()
    g = torch.Generator().manual_seed(R + n_emb)
    dirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
    idx_full = torch.randint(0, n_emb, (R, 2), generator=g).to(dev)
    idx = idx_full[:, 1]  # strided indices (a column of a wider tensor)
    w = torch.randn(n_emb, E, generator=g).to(dev).requires_grad_(True)
    rgb_rows, sky_rows = fused.ray_inputs(w, idx, dirs, max_deg)
    P = 3 if max_deg == 0 else 3 * (1 + 2 * (max_deg + 1))
    assert rgb_rows.shape == (R, P + E) and sky_rows.shape == (R, P + E)
    assert torch.equal(rgb_rows[:, :P], ops.dir_encode(dirs, max_deg, remap=True))
    assert torch.equal(sky_rows[:, :P], ops.dir_encode(dirs, max_deg, remap=False))
    assert torch.equal(rgb_rows[:, P:], w.detach()[idx]) and torch.equal(sky_rows[:, P:], w.detach()[idx])
    ga = torch.randn(R, P + E, generator=g).to(dev)
    gb = torch.randn(R, P + E, generator=g).to(dev)
    ref = torch.zeros(n_emb, E, dtype=torch.float64, device=dev).index_add_(0, idx, (ga[:, P:] + gb[:, P:]).double())
    (dw,) = torch.autograd.grad([rgb_rows, sky_rows], [w], [ga, gb], retain_graph=True)
    assert (dw.double() - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())
    mag = torch.zeros(n_emb, E, dtype=torch.float64, device=dev).index_add_(0, idx, ga[:, P:].abs().double() + gb[:, P:].abs().double())
    assert_bound(dw.cpu().numpy(), ref.cpu().numpy(), mag.cpu().numpy(), c_embed_grad(R), f"embed_grad R={R} n_emb={n_emb} E={E}")
    (dw2,) = torch.autograd.grad([rgb_rows, sky_rows], [w], [ga, gb], retain_graph=True)
    assert torch.equal(dw, dw2)
    (dw_one,) = torch.autograd.grad([sky_rows], [w], [gb])  # one consumer only (eval of the sky head alone)
    ref_one = torch.zeros(n_emb, E, dtype=torch.float64, device=dev).index_add_(0, idx, gb[:, P:].double())
    assert (dw_one.double() - ref_one).abs().max().item() <= 1e-6 * max(1.0, ref_one.abs().max().item())
    mag_one = torch.zeros(n_emb, E, dtype=torch.float64, device=dev).index_add_(0, idx, gb[:, P:].abs().double())
    assert_bound(dw_one.cpu().numpy(), ref_one.cpu().numpy(), mag_one.cpu().numpy(), c_embed_grad(R), f"embed_grad (one consumer) R={R} n_emb={n_emb} E={E}")


def test_ray_inputs_out_of_range_index_poisons_the_row(hip_lib):
    from emernerf_amd import fused
    dev = _dev()
    dirs = torch.nn.functional.normalize(torch.randn(8, 3), dim=-1).to(dev)
    idx = torch.tensor([0, 1, 2, 3, 4, 5, 6, 2], device=dev)
    w = torch.randn(5, 16, device=dev)
    rgb_rows, _ = fused.ray_inputs(w, idx, dirs, 4)
    bad = torch.isnan(rgb_rows[:, 33:]).all(dim=1)
    assert bad.tolist() == [False, False, False, False, False, True, True, False]


@pytest.mark.parametrize("R,Kh,H", [(8192, 49, 64), (45, 33, 64), (1000, 64, 64), (70, 7, 16)])
def test_ray_pre_matches_fp64(hip_lib, R, Kh, H):
    """emer_ray_pre_fwd / bwd against fp64 matmuls on the same column blocks of wider weight matrices (1e-6 relative to the
    largest entry: fp32 dot products of <= 128 terms; per entry within c_ray_pre_fwd(Kh) / c_ray_pre_bwd(H) u (sum |w| |h| +
    |bias|), tests/_bounds.py).  Bit for bit on exact probes: tests/test_ray_exact_gpu.py."""
    import ctypes
    from emernerf_amd import _lib
    dev = _dev()
    g = torch.Generator().manual_seed(R + Kh)
    NG = 64
    W0 = torch.randn(H, Kh + NG, generator=g).to(dev)
    W1 = torch.randn(H, H + Kh + NG, generator=g).to(dev)
    b0, b1 = torch.randn(H, generator=g).to(dev), torch.randn(H, generator=g).to(dev)
    h = torch.randn(R, Kh, generator=g).to(dev)
    rb = torch.empty(R, 2 * H, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wb = W1[:, H:]
    _lib.call("emer_ray_pre_fwd", h.data_ptr(), h.stride(0), R, Kh, H, W0.data_ptr(), W0.stride(0), b0.data_ptr(), wb.data_ptr(), W1.stride(0),
              b1.data_ptr(), rb.data_ptr(), 2 * H, st)
    ref = torch.cat([h.double() @ W0[:, :Kh].double().T + b0.double(), h.double() @ W1[:, H:H + Kh].double().T + b1.double()], 1)
    assert (rb.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    mag = torch.cat([h.abs().double() @ W0[:, :Kh].abs().double().T + b0.abs().double(), h.abs().double() @ W1[:, H:H + Kh].abs().double().T + b1.abs().double()], 1)
    assert_bound(rb.cpu().numpy(), ref.cpu().numpy(), mag.cpu().numpy(), c_ray_pre_fwd(Kh), f"ray_pre_fwd R={R} Kh={Kh} H={H}")
    s0, s1 = torch.randn(R, H, generator=g).to(dev), torch.randn(R, H, generator=g).to(dev)
    dh = torch.empty(R, Kh, device=dev)
    _lib.call("emer_ray_pre_bwd", s0.data_ptr(), s1.data_ptr(), H, R, Kh, H, W0.data_ptr(), W0.stride(0), wb.data_ptr(), W1.stride(0),
              dh.data_ptr(), Kh, st)
    ref = s0.double() @ W0[:, :Kh].double() + s1.double() @ W1[:, H:H + Kh].double()
    assert (dh.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    mag = s0.abs().double() @ W0[:, :Kh].abs().double() + s1.abs().double() @ W1[:, H:H + Kh].abs().double()
    assert_bound(dh.cpu().numpy(), ref.cpu().numpy(), mag.cpu().numpy(), c_ray_pre_bwd(H), f"ray_pre_bwd R={R} Kh={Kh} H={H}")


@pytest.mark.parametrize("M", [8192, 300, 1])
def test_ray_wgrad_matches_fp64(hip_lib, M):
    """emer_ray_wgrad: several per-ray layers' weight / bias gradients in one launch, accumulated into column blocks of wider
    matrices, against fp64 (2e-6 relative to the largest entry: fp32 sums over <= 8192 rows in chunk order; per entry within
    c_ray_wgrad(M) u (sum |dy| |x| + |target|), tests/_bounds.py).  Bit for bit on exact probes: tests/test_ray_exact_gpu.py."""
    from emernerf_amd import fused
    dev = _dev()
    g = torch.Generator().manual_seed(M)
    H, K0, C = 64, 49, 3
    a1, a2, x = (torch.randn(M, w, generator=g).to(dev) for w in (H, H, K0))
    d2, d1, d0 = (torch.randn(M, w, generator=g).to(dev) for w in (C, H, H))
    wide = torch.randn(M, 200, generator=g).to(dev)  # a strided operand (columns 7..56 of a wider tensor)
    xs = wide[:, 7:7 + K0]
    dw2, dw1, dw0 = torch.ones(C, H, device=dev), torch.ones(H, H + K0 + 10, device=dev), torch.ones(H, K0, device=dev)
    db2, db1 = torch.ones(C, device=dev), torch.ones(H, device=dev)
    fused.ray_wgrad([(d2, [(a2, H, 0)], dw2, db2), (d1, [(a1, H, 0), (xs, K0, H + 10)], dw1, db1), (d0, [(x, K0, 0)], dw0, None)], x)

    def chk(got, want, mag, what):
        assert (got.double() - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item())
        # per entry: c u (sum |dy| |x| + the preloaded 1); an untouched column (mag = the preloaded 1 alone) stays within its ulp
        assert_bound(got.cpu().numpy(), want.cpu().numpy(), mag.cpu().numpy(), c_ray_wgrad(M), f"ray_wgrad {what} M={M}")

    ab = lambda t: t.abs().double()
    chk(dw2, 1.0 + d2.double().T @ a2.double(), 1.0 + ab(d2).T @ ab(a2), "dW2")
    chk(db2, 1.0 + d2.double().sum(0), 1.0 + ab(d2).sum(0), "db2")
    want1 = torch.ones(H, H + K0 + 10, dtype=torch.float64, device=dev)
    want1[:, :H] += d1.double().T @ a1.double()
    want1[:, H + 10:] += d1.double().T @ xs.double()
    mag1 = torch.ones(H, H + K0 + 10, dtype=torch.float64, device=dev)
    mag1[:, :H] += ab(d1).T @ ab(a1)
    mag1[:, H + 10:] += ab(d1).T @ ab(xs)
    chk(dw1, want1, mag1, "dW1")  # columns H .. H+10 untouched
    assert bool((dw1[:, H:H + 10] == 1.0).all()), "columns between the blocks must stay as they were"
    chk(db1, 1.0 + d1.double().sum(0), 1.0 + ab(d1).sum(0), "db1")
    chk(dw0, 1.0 + d0.double().T @ x.double(), 1.0 + ab(d0).T @ ab(x), "dW0")


@pytest.mark.parametrize("N,C", [(1000, 64), (3, 4), (4096, 64)])
def test_aggregate3_matches_the_reference_expression(hip_lib, N, C):
    """emer_aggregate3: (cur + 0.5 fwd + 0.5 bwd) / 2 of a [cur | fwd | bwd] batch, bit for bit the reference's expression
    (radiance_field.py:595-613), and its backward [g/2 | g/4 | g/4]."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(N + C)
    x3 = torch.randn(3 * N, C, generator=g).to(dev).requires_grad_(True)
    out = ops.aggregate3(x3)
    cur, fwd, bwd = x3.detach().split(N, dim=0)
    assert torch.equal(out, (cur + 0.5 * fwd + 0.5 * bwd) / 2.0)
    up = torch.randn(N, C, generator=g).to(dev)
    (dx,) = torch.autograd.grad(out, x3, up)
    assert torch.equal(dx, torch.cat([up / 2.0, 0.5 * (up / 2.0), 0.5 * (up / 2.0)], 0))


@pytest.mark.parametrize("R,S,with_rgb,with_sky", [(513, 128, True, True), (64, 48, True, False), (300, 200, False, False), (8192, 128, True, True)])
def test_composite_rgb_equals_the_three_kernel_rendering(hip_lib, R, S, with_rgb, with_sky):
    """[r4] emer_composite_rgb_fwd/bwd (the static model's `rendering` as one launch each way) against render_weights ->
    accumulate_along_rays -> ray_epilogue: outputs bitwise equal, gradients of density / colour / sky colour equal to fp32 rounding,
    including gradients that reach the extras (weights, trans) from other consumers and rays whose opacity sits on the clamp."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(31)
    ts = torch.sort(torch.rand(R, S + 1, generator=g) * 6, dim=-1).values
    t0, t1 = ts[:, :-1].contiguous().to(dev), ts[:, 1:].contiguous().to(dev)
    sig = (torch.rand(R, S, generator=g) * 3).pow(3)
    sig[0] = 0.0          # opacity below the clamp's lower bound
    sig[1] = 50.0         # saturated
    rgb = torch.rand(R, S, 3, generator=g)
    sky = torch.rand(R, 3, generator=g)
    ups = {k: torch.randn(*shape, generator=g).to(dev) for k, shape in
           {"rgb": (R, 3), "opa": (R, 1), "dep": (R, 1), "w": (R, S), "T": (R, S)}.items()}
    res = {}
    for fused in (False, True):
        sg = sig.to(dev).requires_grad_(True)
        c = rgb.to(dev).requires_grad_(True) if with_rgb else None
        sk = sky.to(dev).requires_grad_(True) if (with_rgb and with_sky) else None
        if fused:
            w, T, tm, td, opa, dep, med, out = ops.composite_rgb(t0, t1, sg, c, sk)
        else:
            w, T, _, _, stats, tm, td = ops.render_weights(t0, t1, sg, want_t=True)
            acc = ops.accumulate_along_rays(w, c) if c is not None else None
            opa, dep, med, out = ops.ray_epilogue(stats, acc, sk if acc is not None else None)
        loss = (opa * ups["opa"]).sum() + (dep * ups["dep"]).sum() + (w * ups["w"]).sum() + (T * ups["T"]).sum()
        if out is not None:
            loss = loss + (out * ups["rgb"]).sum()
        loss.backward()
        res[fused] = ([w, T, tm, td, opa, dep, med] + ([out] if out is not None else []),
                      [sg.grad] + ([c.grad] if c is not None else []) + ([sk.grad] if sk is not None else []))
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(res[False][1], res[True][1]):
        scale = a.abs().max().item() + 1e-30
        assert (a - b).abs().max().item() <= 2e-6 * scale, f"gradient differs: {(a - b).abs().max().item():.3e} of {scale:.3e}"
    # the fused kernel against the fp64 restatement itself, entry by entry (a slip shared with the three kernels shows here)
    if R <= 513:
        n = lambda t: t.detach().cpu().numpy()   # noqa: E731
        p = dict(ts=n(t0), te=n(t1), sg=sig.numpy(), rgb=rgb.numpy() if with_rgb else None, sky=sky.numpy() if (with_rgb and with_sky) else None,
                 dW=n(ups["w"]), dT=n(ups["T"]), d_opa=n(ups["opa"]), d_dep=n(ups["dep"]), d_out=n(ups["rgb"]) if with_rgb else None)
        outs, grads = res[True]
        got = dict(weights=n(outs[0]), trans=n(outs[1]), t_mid=n(outs[2]), t_dist=n(outs[3]), opacity=n(outs[4])[:, 0], depth=n(outs[5])[:, 0],
                   median=n(outs[6])[:, 0], rgb_out=n(outs[7]) if with_rgb else None, d_sigma=n(grads[0]),
                   d_rgb=n(grads[1]) if with_rgb else None, d_sky=n(grads[2]) if (with_rgb and with_sky) else None)
        CP.check_real_composite(p, got, f"composite_rgb R={R} S={S}", allow_ambiguous=True, wsum=n(stats)[:, 0])


@pytest.mark.parametrize("R,S,C", [(257, 128, 64), (33, 50, 100), (2048, 128, 64)])
def test_blend_accumulate_wide_matches_the_reference_expression(hip_lib, R, S, C):
    """[r4] emer_blend_accumulate_wide_fwd/bwd against the reference's own expression (render_utils.py:131-136,247-252) in fp64."""
    from emernerf_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(41)
    w = torch.rand(R, S, generator=g) / S
    ss, sd = torch.rand(R, S, 1, generator=g).pow(3) * 5, torch.rand(R, S, 1, generator=g).pow(3) * 5
    ss[0] = 0.0
    sd[0] = 0.0   # density 0: ratios 0 / 1e-6
    fs, fd = torch.randn(R, S, C, generator=g), torch.randn(R, S, C, generator=g)
    up = torch.randn(R, C, generator=g)
    leaves = [t.to(dev).requires_grad_(True) for t in (w, ss, sd, fs, fd)]
    sg = leaves[1] + leaves[2]
    sg.retain_grad()
    acc = ops.blend_accumulate_wide(leaves[0], sg, leaves[1], leaves[2], leaves[3], leaves[4])
    (acc * up.to(dev)).sum().backward()
    ref = [t.double().requires_grad_(True) for t in (w, ss, sd, fs, fd)]
    rsg = ref[1] + ref[2]
    rsg.retain_grad()
    feat = (ref[1] / (rsg + 1e-6)) * ref[3] + (ref[2] / (rsg + 1e-6)) * ref[4]
    racc = (ref[0][..., None] * feat).sum(1)
    (racc * up.double()).sum().backward()
    np.testing.assert_allclose(acc.detach().cpu().numpy(), racc.detach().numpy(), rtol=0, atol=2e-6 * float(racc.abs().max()))
    for a, b, name in zip(leaves + [sg], ref + [rsg], ["w", "sigma_s", "sigma_d", "feat_s", "feat_d", "sigma"]):
        scale = float(b.grad.abs().max()) + 1e-30
        err = float((a.grad.cpu().double() - b.grad).abs().max())
        assert err <= 5e-6 * scale, f"d {name}: {err:.3e} of {scale:.3e}"
    if R <= 257:   # per entry (tests/_bounds.py blend_c)
        n = lambda t: t.detach().cpu().numpy()   # noqa: E731
        p = dict(w=w.numpy(), sig=n(sg)[..., 0], ss=ss.numpy()[..., 0], sd=sd.numpy()[..., 0], fs=fs.numpy(), fd=fd.numpy(), g_acc=up.numpy())
        got = dict(acc=n(acc), d_w=n(leaves[0].grad), d_ss=n(leaves[1].grad)[..., 0], d_sd=n(leaves[2].grad)[..., 0], d_fs=n(leaves[3].grad),
                   d_fd=n(leaves[4].grad), d_sig=n(sg.grad)[..., 0])
        CP.check_real_blend_through_sum(p, got, f"blend wide R={R} S={S} C={C}", wide=True)


