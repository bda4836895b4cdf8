"""Every (D, F) instantiation of the grid kernels, every route: exact probes, per-entry bounds for the fp32 atomic backward, the
fp16-table input gradient and the half atomics, and the Python routes that reach them.

Exact probes (tests/_grid_probe.py): all sums are exact in any order, so every kernel must equal the double-precision oracle
BITWISE -- forward (fp32 / fp16 table, both layouts, the Jacobian forward), the gather input gradient (fp32 / fp16 table, both
dOut layouts), the stored-Jacobian input gradient (rows from 0 and from n // 3), the fp32 and half atomic table gradients (both
layouts), the owner-computes table gradient and its accumulating variant.  tests/test_hashgrid_instances_cpu.py proves the
premises.

Random data (n = 4099, the edge rows of tests/test_kernels_gpu._inputs) on every grid of GRIDS: the per-entry bounds of
tests/_bounds.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _grid_probe as GP
from tests._bounds import (U, assert_bound, assert_err_bound, c_atomic, c_forward, c_input_grad, c_sliced, fp16_atomic_bound,
                           half_rounded_bound)
from tests.test_kernels_gpu import GRIDS, _dev, _inputs, _mk

pytestmark = pytest.mark.gpu

EVEN_GRIDS = [name for name, cfg in GRIDS.items() if cfg[5] % 2 == 0]
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ direct ABI calls
def _strides(desc, n, row_major):
    L, F = desc.n_levels, desc.n_features
    return (L * F, F) if row_major else (F, n * F)


def _tag(t):
    from emernerf_amd import _lib
    return _lib.F32 if t.dtype == torch.float32 else _lib.F16


def _call(name, t, *args):
    from emernerf_amd import _lib
    with torch.cuda.device(t.device):
        _lib.call(name, *args, _lib._stream(t))


def _bwd_input(desc, x, table, dout, row_major):
    """emer_hashgrid_bwd_input into a NaN-filled dx; dout: the [n, L*F] (row_major) or [L, n, F] device tensor"""
    n = x.shape[0]
    dx = torch.full((n, desc.n_dims), NAN, device=x.device)
    sn, sl = _strides(desc, n, row_major)
    _call("emer_hashgrid_bwd_input", x, ctypes.byref(desc), x.data_ptr(), table.data_ptr(), _tag(table), dout.data_ptr(), sn, sl, dx.data_ptr(), n)
    return dx


def _bwd_input_jac(desc, jac, dout, row_major, n, row0):
    """emer_hashgrid_bwd_input_jac for the rows row0 .. n - 1 of dout"""
    rows = n - row0
    dx = torch.full((rows, desc.n_dims), NAN, device=dout.device)
    sn, sl = _strides(desc, n, row_major)
    _call("emer_hashgrid_bwd_input_jac", dout, ctypes.byref(desc), jac.data_ptr(), dout.data_ptr() + 4 * row0 * sn, sn, sl, dx.data_ptr(), rows)
    return dx


def _bwd_params(desc, x, dout, row_major, dtype=torch.float32):
    """emer_hashgrid_bwd_params (global atomics) into a zeroed table of ``dtype``"""
    n = x.shape[0]
    grad = torch.zeros(desc.n_entries * desc.n_features, device=x.device, dtype=dtype)
    sn, sl = _strides(desc, n, row_major)
    _call("emer_hashgrid_bwd_params", x, ctypes.byref(desc), x.data_ptr(), dout.data_ptr(), sn, sl, grad.data_ptr(), _tag(grad), n)
    return grad


def _bwd_sliced(desc, x, dout_lm, grad=None, add=False):
    """emer_hashgrid_bwd_params_sliced[_add] (owner computes); a fresh gradient table is NaN-filled: every entry must be written"""
    from emernerf_amd import ops
    n = x.shape[0]
    assert ops.sliced_supported(desc)
    if grad is None:
        grad = torch.full((desc.n_entries * desc.n_features,), NAN, device=x.device)
    masks = ops.slice_masks(desc, x)
    F = desc.n_features
    _call("emer_hashgrid_bwd_params_sliced_add" if add else "emer_hashgrid_bwd_params_sliced", x, ctypes.byref(desc), x.data_ptr(), dout_lm.data_ptr(), F,
          n * F, masks.data_ptr(), grad.data_ptr(), n)
    return grad


# ----------------------------------------------------------------------------------------------------- exact probes
def _probe(oracle, D, F, log2_T, n, sparse=False):
    meta, desc = GP._exact_grid(oracle, F, log2_T, D)
    x, p = GP._probe_positions(n, D), GP._probe_table(meta, GP.table_seed(D, F, log2_T))
    dout = GP.probe_dout(n, meta.n_levels, F, 7 * n + D, sparse=sparse)
    return meta, desc, x, p, dout


PROBES = pytest.mark.parametrize("D,F,log2_T", [(D, F, T) for D in GP.DIMS for F in GP.FEATURES for T in GP.LOG2_T])


@PROBES
@pytest.mark.parametrize("n", GP.COUNTS)
def test_probe_forward_is_the_oracle_bitwise(hip_lib, oracle, D, F, log2_T, n):
    """emer_hashgrid_fwd with the fp32 table and its fp16 copy, row-major and level-major, and the Jacobian forward's encoding"""
    from emernerf_amd import ops
    meta, desc, x, p, _ = _probe(oracle, D, F, log2_T, n)
    ref = oracle.hashgrid_fwd_bound(meta, x, p)[0]
    dev = _dev()
    xd, pd = x.to(dev), p.to(dev)
    for tag, table in (("fp32", pd), ("fp16", pd.half())):
        rm = ops.hashgrid_fwd_raw(desc, xd, table, level_major=False)
        GP.assert_bits(rm, ref, f"forward, {tag} table, row-major")
        lm = ops.hashgrid_fwd_raw(desc, xd, table, level_major=True)
        assert torch.equal(lm.permute(1, 0, 2).reshape(n, -1), rm), f"forward, {tag} table: level-major differs from row-major"
    for level_major in (False, True):
        enc, _ = ops.hashgrid_fwd_raw(desc, xd, pd, level_major=level_major, jac_row0=0)
        enc = enc.permute(1, 0, 2).reshape(n, -1) if level_major else enc
        GP.assert_bits(enc, ref, f"Jacobian forward's encoding, level_major={level_major}")


@PROBES
@pytest.mark.parametrize("n", GP.COUNTS)
def test_probe_input_gradient_is_the_oracle_bitwise(hip_lib, oracle, D, F, log2_T, n):
    """emer_hashgrid_bwd_input (fp32 table and its fp16 copy) and emer_hashgrid_fwd_jac + emer_hashgrid_bwd_input_jac (rows from 0
    and from n // 3), each with level-major and row-major dOut strides"""
    from emernerf_amd import ops
    meta, desc, x, p, dout = _probe(oracle, D, F, log2_T, n)
    ref = oracle.hashgrid_bwd_input_bound(meta, x, p, dout)[0]
    dev = _dev()
    xd, pd = x.to(dev), p.to(dev)
    d_rm = dout.to(dev)
    d_lm = GP.level_major(dout, meta.n_levels, F).to(dev)
    for tag, table in (("fp32", pd), ("fp16", pd.half())):
        got = {}
        for row_major, d in ((False, d_lm), (True, d_rm)):
            got[row_major] = _bwd_input(desc, xd, table, d, row_major)
            GP.assert_bits(got[row_major], ref, f"gather input gradient, {tag} table, row_major={row_major}")
        assert torch.equal(got[False], got[True])
    for row0 in sorted({0, n // 3}):
        _, jac = ops.hashgrid_fwd_raw(desc, xd, pd, level_major=True, jac_row0=row0)
        got = {}
        for row_major, d in ((False, d_lm), (True, d_rm)):
            got[row_major] = _bwd_input_jac(desc, jac, d, row_major, n, row0)
            GP.assert_bits(got[row_major], ref[row0:], f"stored-Jacobian input gradient, jac_row0={row0}, row_major={row_major}")
        assert torch.equal(got[False], got[True])


@PROBES
@pytest.mark.parametrize("n", GP.COUNTS)
def test_probe_table_gradient_is_the_oracle_bitwise(hip_lib, oracle, D, F, log2_T, n):
    """emer_hashgrid_bwd_params (fp32 atomics, both dOut layouts, zeroed table), emer_hashgrid_bwd_params_sliced (NaN-filled table),
    and sliced followed by sliced_add of the same launch: exactly twice the gradient"""
    meta, desc, x, p, dout = _probe(oracle, D, F, log2_T, n)
    ref = oracle.hashgrid_bwd_params_bound(meta, x, dout)[0]
    dev = _dev()
    xd = x.to(dev)
    d_rm = dout.to(dev)
    d_lm = GP.level_major(dout, meta.n_levels, F).to(dev)
    got = {}
    for row_major, d in ((False, d_lm), (True, d_rm)):
        got[row_major] = _bwd_params(desc, xd, d, row_major)
        GP.assert_bits(got[row_major], ref, f"fp32 atomic table gradient, row_major={row_major}")
    assert torch.equal(got[False], got[True])
    sliced = _bwd_sliced(desc, xd, d_lm)
    GP.assert_bits(sliced, ref, "owner-computes table gradient")
    twice = _bwd_sliced(desc, xd, d_lm, grad=sliced.clone(), add=True)
    GP.assert_bits(twice, 2.0 * ref, "owner-computes table gradient, sliced + sliced_add")


@pytest.mark.parametrize("D,F,log2_T", [(D, F, T) for D in GP.DIMS for F in GP.FEATURES if F % 2 == 0 for T in GP.LOG2_T])
@pytest.mark.parametrize("n", GP.HALF_COUNTS)
def test_probe_half_table_gradient_is_the_oracle_bitwise(hip_lib, oracle, D, F, log2_T, n):
    """emer_hashgrid_bwd_params with EMER_F16 (packed half2 atomics) on the sparse probe, both dOut layouts"""
    meta, desc, x, p, dout = _probe(oracle, D, F, log2_T, n, sparse=True)
    ref = oracle.hashgrid_bwd_params_bound(meta, x, dout)[0]
    dev = _dev()
    xd = x.to(dev)
    for row_major, d in ((False, GP.level_major(dout, meta.n_levels, F).to(dev)), (True, dout.to(dev))):
        got = _bwd_params(desc, xd, d, row_major, dtype=torch.float16)
        GP.assert_bits(got, ref, f"half atomic table gradient, row_major={row_major}")


# ------------------------------------------------------------------------------------- random data, per-entry bounds
@pytest.mark.parametrize("name", list(GRIDS))
def test_fp32_atomics_within_c_atomic(hip_lib, oracle, name):
    """hashgrid_bwd_params_kernel<D, F, float> through emer_hashgrid_bwd_params(EMER_F32), level-major and row-major dOut: every
    entry within c_atomic(D, hits), untouched entries exactly 0"""
    meta, desc = _mk(oracle, name)
    n = GP.RANDOM_N
    x, _ = _inputs(meta, n, 3)
    dout = GP.random_dout(meta, n, 20)
    g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    dev = _dev()
    xd = x.to(dev)
    for row_major, d in ((False, GP.level_major(dout, meta.n_levels, meta.n_features).to(dev)), (True, dout.to(dev))):
        got = _bwd_params(desc, xd, d, row_major).cpu().numpy()
        assert not got[gabs == 0].any(), "an untouched entry is not exactly 0"
        assert_bound(got, g64, gabs, c_atomic(meta.n_dims, hits), f"fp32 atomics {name} row_major={row_major}", meta=meta, hits=hits)


@pytest.mark.parametrize("name", list(GRIDS))
def test_fp16_table_input_gradient_within_c_input_grad(hip_lib, oracle, name):
    """hashgrid_bwd_input_kernel<D, F, __half>: the half-to-float conversion of an entry is exact, so the fp32 constant stands
    against the oracle on the rounded table"""
    meta, desc = _mk(oracle, name)
    n = GP.RANDOM_N
    x, p = _inputs(meta, n, 3)
    dout = GP.random_dout(meta, n, 20)
    ph = p.half()
    dx64, bx = oracle.hashgrid_bwd_input_bound(meta, x, ph.float(), dout)
    dev = _dev()
    xd, td = x.to(dev), ph.to(dev)
    got = {}
    for row_major, d in ((False, GP.level_major(dout, meta.n_levels, meta.n_features).to(dev)), (True, dout.to(dev))):
        got[row_major] = _bwd_input(desc, xd, td, d, row_major)
        assert_bound(got[row_major].cpu().numpy(), dx64, bx, c_input_grad(meta.n_dims, meta.n_levels, meta.n_features),
                     f"fp16-table input gradient {name} row_major={row_major}", meta=meta, kind="dx")
    assert torch.equal(got[False], got[True])


@pytest.mark.parametrize("name", EVEN_GRIDS)
def test_fp16_atomics_within_the_bound(hip_lib, oracle, name):
    """hashgrid_bwd_params_kernel<D, F, __half> on gradients of order 1 - 10: every value within fp16_atomic_bound (derived in
    tests/_bounds.py; test_half_gradient_inputs_stay_in_range proves its range conditions), untouched entries exactly 0"""
    meta, desc = _mk(oracle, name)
    n = GP.RANDOM_N
    x, _ = _inputs(meta, n, 3)
    dout = GP.random_dout(meta, n, 21, loss_scaled=True)
    g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    bound = fp16_atomic_bound(meta.n_dims, hits, gabs)
    dev = _dev()
    xd = x.to(dev)
    for row_major, d in ((False, GP.level_major(dout, meta.n_levels, meta.n_features).to(dev)), (True, dout.to(dev))):
        got = _bwd_params(desc, xd, d, row_major, dtype=torch.float16).float().cpu().numpy()
        assert np.isfinite(got).all()
        assert_err_bound(got, g64, bound, f"fp16 atomics {name} row_major={row_major}")


# ---------------------------------------------------------------------------------------------------- Python routes
def _small_grid(oracle, D, F):
    from emernerf_amd import _lib
    L, base, mx, T = (4, 4, 32, 12) if D == 4 else (4, 4, 64, 10) if D == 3 else (5, 8, 256, 12)
    meta = oracle.grid_meta_from_encoder_args(D, L, base, mx, T, F)
    return meta, _lib.make_grid_desc(D, L, F, T, base, meta.per_level_scale), dict(
        otype="HashGrid", n_levels=L, n_features_per_level=F, log2_hashmap_size=T, base_resolution=base, per_level_scale=meta.per_level_scale)


@pytest.mark.parametrize("k", [0, 100])
def test_encode_lm_fp16_table_input_gradient(hip_lib, oracle, k):
    """ops.hashgrid_encode_lm(table_dtype=float16, skip_dx_rows=k) with positions that need a gradient: the only input-gradient
    route of fp16 tables is the gather kernel on the fp16 copy, called with pointers offset by k rows"""
    from emernerf_amd import ops
    meta, desc, _ = _small_grid(oracle, 4, 4)
    n, L, F, D = 300, meta.n_levels, meta.n_features, meta.n_dims
    x, p = _inputs(meta, n, 31)
    dout = GP.random_dout(meta, n, 32)
    dev = _dev()
    d_lm = GP.level_major(dout, L, F).to(dev)
    xd = x.to(dev).requires_grad_(True)
    pm = p.to(dev).requires_grad_(True)
    assert ops.sliced_supported(desc)
    lm = ops.hashgrid_encode_lm(xd, pm, desc, table_dtype=torch.float16, skip_dx_rows=k)
    lm.backward(d_lm)
    ph = p.half()
    f64, fabs_ = oracle.hashgrid_fwd_bound(meta, x, ph.float())
    assert_bound(lm.detach().permute(1, 0, 2).reshape(n, -1).cpu().numpy(), f64, fabs_, c_forward(D), f"encode_lm fp16 table k={k}: encoding", meta=meta, kind="fwd")
    dx = xd.grad
    assert dx.dtype == torch.float32 and not dx[:k].any(), "skipped rows must get an exactly zero gradient"
    dx64, bx = oracle.hashgrid_bwd_input_bound(meta, x, ph.float(), dout)
    dx64[:k] = 0.0
    bx[:k] = 0.0
    assert_bound(dx.cpu().numpy(), dx64, bx, c_input_grad(D, L, F), f"encode_lm fp16 table k={k}: input gradient", meta=meta, kind="dx")
    direct = _bwd_input(desc, x.to(dev), ph.to(dev), d_lm, False)
    assert torch.equal(dx[k:], direct[k:]), "not bitwise the direct fp16 emer_hashgrid_bwd_input call on the cast table"
    assert pm.grad.dtype == torch.float32
    g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    assert_bound(pm.grad.cpu().numpy(), g64, gabs, c_sliced(meta, desc, hits), f"encode_lm fp16 table k={k}: master gradient", meta=meta, hits=hits)


def _encoding(cfg, D, p, dev):
    from emernerf_amd.tcnn_modules import Encoding
    enc = Encoding(D, cfg, dtype=torch.float16).to(dev)
    with torch.no_grad():
        enc.params.copy_(p.to(dev))
    return enc


@pytest.mark.parametrize("D,F", [(2, 2), (3, 8), (4, 4)])
def test_encoding_fp16_forward_and_half_gradient(hip_lib, oracle, D, F):
    """Encoding(dtype=float16).forward on an even-F grid: the table is rounded to half, the gradient comes from the half atomics
    and is handed to the fp32 master through the cast's backward"""
    meta, desc, cfg = _small_grid(oracle, D, F)
    n = 1000
    x, p = _inputs(meta, n, 41)
    dout = GP.random_dout(meta, n, 42, loss_scaled=True)
    dev = _dev()
    enc = _encoding(cfg, D, p, dev)
    out = enc(x.to(dev))
    out.backward(dout.to(dev))
    f64, fabs_ = oracle.hashgrid_fwd_bound(meta, x, p.half().float())
    assert_bound(out.detach().cpu().numpy(), f64, fabs_, c_forward(D), f"Encoding fp16 D={D} F={F}: encoding", meta=meta, kind="fwd")
    g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    assert enc.params.grad.dtype == torch.float32
    assert_err_bound(enc.params.grad.cpu().numpy(), g64, fp16_atomic_bound(D, hits, gabs, extra=1), f"Encoding fp16 D={D} F={F}: table gradient")


@pytest.mark.parametrize("D", GP.DIMS)
def test_encoding_fp16_odd_feature_count_has_a_gradient(hip_lib, oracle, D):
    """Half gradients with one feature per level (every proposal network): there is no packed half atomic for an odd feature
    count, so both autograd functions accumulate in fp32 (owner computes here) and cast to half once: the fp32 bound plus one
    half rounding."""
    from emernerf_amd import ops
    meta, desc, cfg = _small_grid(oracle, D, 1)
    n = 1000
    x, p = _inputs(meta, n, 51)
    dev = _dev()
    assert ops.sliced_supported(desc)

    def check(grad, dout, what):
        g64, gabs, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
        assert grad.dtype == torch.float32 and torch.equal(grad.half().float(), grad), "the gradient was not rounded to half"
        err = half_rounded_bound(c_sliced(meta, desc, hits) * U * gabs, g64)
        assert_err_bound(grad.cpu().numpy(), g64, err, what)

    enc = _encoding(cfg, D, p, dev)
    enc(x.to(dev)).sum().backward()
    check(enc.params.grad, torch.ones(n, meta.n_output_dims), f"Encoding fp16 D={D} F=1: table gradient")
    # the level-major function, with an fp16 table and half gradients
    dout = GP.random_dout(meta, n, 52)
    pm = p.to(dev).requires_grad_(True)
    lm = ops.hashgrid_encode_lm(x.to(dev), pm.half(), desc, grad_dtype=torch.float16)
    lm.backward(GP.level_major(dout, meta.n_levels, 1).to(dev))
    check(pm.grad, dout, f"encode_lm fp16 gradients D={D} F=1: table gradient")


def test_grid_entry_points_refuse_bad_arguments_before_any_launch(hip_lib, oracle):
    """param_dtype / grad_dtype = 2, half gradients with an odd feature count: an error, and the sentinel-filled output is
    untouched; n = 0: OK, and the output is untouched"""
    from emernerf_amd import _lib
    dev = _dev()
    n = 65
    for F in (1, 2):
        meta, desc, _ = _small_grid(oracle, 3, F)
        x, p = _inputs(meta, n, 61)
        xd, pd = x.to(dev), p.to(dev)
        L = meta.n_levels
        dout = torch.ones(L, n, F, device=dev)
        sn, sl = F, n * F
        out = torch.full((L, n, F), 7.0, device=dev)
        dx = torch.full((n, 3), 7.0, device=dev)
        grad = torch.full((meta.n_params,), 7.0, device=dev)
        gradh = torch.full((meta.n_params,), 7.0, device=dev, dtype=torch.float16)
        jac = torch.full((L, n, F, 3), 7.0, device=dev)
        d = ctypes.byref(desc)
        calls = {
            "fwd": lambda tag, m: _call("emer_hashgrid_fwd", xd, d, xd.data_ptr(), pd.data_ptr(), tag, out.data_ptr(), sn, sl, None, m),
            "bwd_input": lambda tag, m: _call("emer_hashgrid_bwd_input", xd, d, xd.data_ptr(), pd.data_ptr(), tag, dout.data_ptr(), sn, sl, dx.data_ptr(), m),
            "bwd_params": lambda tag, m: _call("emer_hashgrid_bwd_params", xd, d, xd.data_ptr(), dout.data_ptr(), sn, sl,
                                               (gradh if tag == _lib.F16 else grad).data_ptr(), tag, m),
        }
        for name, fn in calls.items():
            with pytest.raises(_lib.EmerError, match="dtype"):
                fn(2, n)
            fn(_lib.F32, 0)
            fn(_lib.F16, 0)
        if F % 2:
            with pytest.raises(_lib.EmerError, match="even n_features"):
                calls["bwd_params"](_lib.F16, n)
        _call("emer_hashgrid_fwd_jac", xd, d, xd.data_ptr(), pd.data_ptr(), out.data_ptr(), sn, sl, None, jac.data_ptr(), 0, 0)
        _call("emer_hashgrid_bwd_input_jac", xd, d, jac.data_ptr(), dout.data_ptr(), sn, sl, dx.data_ptr(), 0)
        torch.cuda.synchronize()
        for t in (out, dx, grad, gradh, jac):
            assert bool((t == 7.0).all()), "an output was written by a call that had to return before any launch"
