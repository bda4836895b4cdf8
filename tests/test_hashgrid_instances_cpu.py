"""The premises of tests/test_hashgrid_instances_gpu.py, proved on the CPU from the double-precision oracle: the exactness
conditions of the probes for every (D, F, log2_T, n) the GPU tests run, what the probes reach, that a swapped feature, a swapped
axis or a misread stride changes the oracle's result on every level, and the range conditions of the half-gradient bound."""
import numpy as np
import pytest
import torch

from tests import _grid_probe as GP
from tests._bounds import HALF_MAX, U16, fp16_atomic_bound, half_rounded_bound


def _case(oracle, D, F, log2_T, n, sparse=False):
    meta, _ = GP._exact_grid(oracle, F, log2_T, D)
    x, p = GP._probe_positions(n, D), GP._probe_table(meta, GP.table_seed(D, F, log2_T))
    dout = GP.probe_dout(n, meta.n_levels, F, 7 * n + D, sparse=sparse)
    return meta, x, p, dout


@pytest.mark.parametrize("log2_T", GP.LOG2_T)
@pytest.mark.parametrize("F", GP.FEATURES)
@pytest.mark.parametrize("D", GP.DIMS)
def test_probe_sums_are_exact_in_any_order(oracle, D, F, log2_T):
    """abs_sum / g < 2^24 for the forward, the table gradient and the input gradient (fp32 accumulators), abs_sum / g < 2^11,
    g >= 2^-24 and abs_sum <= 65504 for the sparse table gradient (half accumulators); every result is an fp32 number and a
    multiple of g."""
    for n in GP.COUNTS:
        meta, x, p, dout = _case(oracle, D, F, log2_T, n)
        assert np.array_equal(meta.scale, np.array([3, 7, 15, 31, 63], np.float32))
        assert torch.equal(p.half().float(), p) and float(p.abs().max()) <= 0.5 and torch.equal(p * 16, (p * 16).round())
        assert torch.equal(x * 4, (x * 4).round())
        assert torch.equal(dout, dout.round()) and float(dout.abs().max()) <= 2
        for what, (ref, abs_sum), g in (("forward", oracle.hashgrid_fwd_bound(meta, x, p), GP.g_forward(D)),
                                        ("table gradient", oracle.hashgrid_bwd_params_bound(meta, x, dout)[:2], GP.g_params(D)),
                                        ("input gradient", oracle.hashgrid_bwd_input_bound(meta, x, p, dout), GP.g_input(D))):
            assert float(abs_sum.max()) / g < 2.0 ** 24, (what, n, float(abs_sum.max()))
            assert np.array_equal(ref / g, np.round(ref / g)) and np.array_equal(abs_sum / g, np.round(abs_sum / g)), f"{what}: no multiples of g"
            GP.exact_f32(ref)
    if F % 2 == 0:
        g = GP.g_params(D)
        assert g >= 2.0 ** -24
        for n in GP.HALF_COUNTS:
            meta, x, p, dout = _case(oracle, D, F, log2_T, n, sparse=True)
            assert float(dout.abs().max()) <= 1
            ref, abs_sum, _ = oracle.hashgrid_bwd_params_bound(meta, x, dout)
            assert float(abs_sum.max()) / g < 2.0 ** 11 and float(abs_sum.max()) <= HALF_MAX, (n, float(abs_sum.max()))
            assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref), "the sparse table gradient is no half number"


@pytest.mark.parametrize("D", GP.DIMS)
def test_probe_reaches_the_cases(oracle, D):
    """Per D: a dense and a hashed level; on every level x beyond the level and x in its last cell (none beyond in the first two
    waves), entries hit more than once; zero and non-zero dOut rows in every wave."""
    dense = hashed = False
    for log2_T in GP.LOG2_T:
        meta, _ = GP._exact_grid(oracle, 2, log2_T, D)
        assert np.array_equal(meta.res, [4, 8, 16, 32, 64])
        dense |= bool((meta.hashed == 0).any())
        hashed |= bool((meta.hashed != 0).any())
        for n in (257, 1000):
            x = GP._probe_positions(n, D)
            dout = GP.probe_dout(n, meta.n_levels, 2, 7 * n + D)
            hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)[2]
            for l in range(meta.n_levels):
                gi, w, pos = GP._cells(meta, x, l)
                assert np.array_equal(pos, pos.astype(np.float32)) and np.array_equal(w * 4, np.round(w * 4))
                res = int(meta.res[l])
                beyond = gi[:, 0] >= res
                assert not beyond[:GP.INSIDE_ROWS].any() and beyond[GP.INSIDE_ROWS:257].any(), f"level {l}: x beyond the level"
                assert (gi[:, 0] == res - 1).any(), f"level {l}: x in the last cell"
                a, b = int(meta.offset[l]), int(meta.offset[l]) + int(meta.size[l])
                assert int(hits[a:b].max()) > 1, f"level {l}: no entry with more than one hit"
    assert dense and hashed
    if D == 4:
        assert GP._exact_grid(oracle, 1, 12, 4)[0].hashed[0] == 0, "no dense 4-D level"
    for sparse in (False, True):
        for n in GP.COUNTS:
            z = (GP.probe_dout(n, 5, 2, 7 * n + D, sparse=sparse) == 0).all(1).numpy()
            assert not z[0]
            for wave in range(0, n - 63, 64):
                assert 0 < z[wave:wave + 64].sum() < 64


@pytest.mark.parametrize("log2_T", GP.LOG2_T)
@pytest.mark.parametrize("F", GP.FEATURES)
@pytest.mark.parametrize("D", GP.DIMS)
def test_probe_sees_a_swapped_feature_axis_or_stride(oracle, D, F, log2_T):
    """The oracle's result changes on EVERY level under a permutation of the table's features, a swap of two position columns
    and a row-major dOut read with level-major strides: a kernel that did one of these could not equal the oracle."""
    for n in (65, 257, 1000):
        meta, x, p, dout = _case(oracle, D, F, log2_T, n)
        L = meta.n_levels
        fwd = oracle.hashgrid_fwd_bound(meta, x, p)[0].reshape(n, L, F)
        grad = oracle.hashgrid_bwd_params_bound(meta, x, dout)[0]
        dx = oracle.hashgrid_bwd_input_bound(meta, x, p, dout)[0]
        lv = GP.level_slices(meta)
        swap = list(range(D))
        swap[0], swap[1] = 1, 0
        xs = x[:, swap].contiguous()
        fwd_s = oracle.hashgrid_fwd_bound(meta, xs, p)[0].reshape(n, L, F)
        grad_s = oracle.hashgrid_bwd_params_bound(meta, xs, dout)[0]
        for l in range(L):
            assert not np.array_equal(fwd_s[:, l], fwd[:, l]), f"level {l}: the forward does not see swapped axes"
            assert not np.array_equal(grad_s[lv[l]], grad[lv[l]]), f"level {l}: the table gradient does not see swapped axes"
        assert not np.array_equal(oracle.hashgrid_bwd_input_bound(meta, xs, p, dout)[0][:, swap], dx)
        if F > 1:
            pr = p.view(-1, F).roll(1, dims=1).reshape(-1).contiguous()
            fwd_r = oracle.hashgrid_fwd_bound(meta, x, pr)[0].reshape(n, L, F)
            dr = dout.view(n, L, F).roll(1, dims=2).reshape(n, L * F).contiguous()
            grad_r = oracle.hashgrid_bwd_params_bound(meta, x, dr)[0]
            for l in range(L):
                assert not np.array_equal(fwd_r[:, l], fwd[:, l]), f"level {l}: the forward does not see permuted features"
                assert not np.array_equal(grad_r[lv[l]], grad[lv[l]]), f"level {l}: the table gradient does not see permuted features"
        mis = GP.misread_as_level_major(dout, L, F)
        grad_m = oracle.hashgrid_bwd_params_bound(meta, x, mis)[0]
        for l in range(L):
            assert not np.array_equal(grad_m[lv[l]], grad[lv[l]]), f"level {l}: the table gradient does not see a misread stride"
        assert not np.array_equal(oracle.hashgrid_bwd_input_bound(meta, x, p, mis)[0], dx), "the input gradient does not see a misread stride"


def _even_grids():
    from tests.test_kernels_gpu import GRIDS
    return [name for name, cfg in GRIDS.items() if cfg[5] % 2 == 0]


def test_all_twelve_instantiations_have_a_grid():
    from tests.test_kernels_gpu import GRIDS
    assert {(cfg[0], cfg[5]) for cfg in GRIDS.values()} == {(D, F) for D in GP.DIMS for F in GP.FEATURES}


@pytest.mark.parametrize("name", _even_grids())
def test_half_gradient_inputs_stay_in_range(oracle, name):
    """The inputs of test_fp16_atomics_within_the_bound: |dOut| in [1, 10], every partial sum below the half overflow, fewer
    than 2047 hits per entry (fp16_atomic_bound asserts both), and the relative part of the bound dominates its absolute part
    on most of the touched values."""
    from tests.test_kernels_gpu import _inputs, _mk
    meta, _ = _mk(oracle, name)
    x, _ = _inputs(meta, GP.RANDOM_N, 3)
    dout = GP.random_dout(meta, GP.RANDOM_N, 21, loss_scaled=True)
    nz = dout[dout != 0].abs()
    assert float(nz.min()) >= 1.0 and float(nz.max()) <= 10.0 and bool((dout == 0).all(1).any())
    _, abs_sum, hits = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    assert float(abs_sum.max()) < HALF_MAX
    bound = fp16_atomic_bound(meta.n_dims, hits, abs_sum)
    touched = abs_sum > 0
    assert bool(touched.any()) and bool((bound[~touched] == 0).all())
    absolute = (np.repeat(hits, meta.n_features) + 1.0) * 2.0 ** -14
    assert float((bound[touched] >= 2 * absolute[touched]).mean()) > 0.5   # (abs_sum >= 1 / 8: all but entries reached by tiny weights only)


def test_fp16_atomic_bound_is_what_its_derivation_says():
    """gamma_k with u = 2^-11 and k = hits + 1, the fp32 term's 2D roundings, (hits + 1) 2^-14 absolute, 0 for an untouched
    entry; k u >= 1 and a possible half overflow are refused."""
    hits = np.array([0, 1, 100], np.uint32)
    abs_sum = np.array([0.0, 0.0, 3.0, 1.0, 50.0, 0.0])
    b = fp16_atomic_bound(3, hits, abs_sum)
    k = 101.0
    gam = k * U16 / (1 - k * U16)
    assert b[0] == 0 and b[1] == 0 and b[5] == 0
    assert b[2] == ((1 + 6 * 2.0 ** -24) * (1 + 2 * U16 / (1 - 2 * U16)) - 1) * 3.0 + 2 * 2.0 ** -14
    assert b[4] == ((1 + 6 * 2.0 ** -24) * (1 + gam) - 1) * 50.0 + 101 * 2.0 ** -14
    assert fp16_atomic_bound(3, hits, abs_sum, extra=1)[4] > b[4]
    with pytest.raises(AssertionError):
        fp16_atomic_bound(3, np.array([2047], np.uint32), np.array([1.0]))
    with pytest.raises(AssertionError):
        fp16_atomic_bound(3, np.array([8], np.uint32), np.array([65504.0]))
    h = half_rounded_bound(np.array([0.0, 1e-3, 1e-9]), np.array([0.0, 2.0, 1e-9]))
    assert h[0] == 0 and h[1] == 1e-3 + U16 * (2.0 + 1e-3) and h[2] == 1e-9 + 2.0 ** -25
