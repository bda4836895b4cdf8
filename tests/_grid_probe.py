"""Exact probes for every (D, F) instantiation of the grid kernels (test helper, not a test module).

The probe of tests/test_hashgrid_pairs_gpu.py, in all dimensions and with gradients: a base-4 grid of per-level scale 2 (level
scales 3, 7, 15, 31, 63), positions that are multiples of 1/4, table entries k / 16 with |k| <= 8 and gradients dOut that are
small integers.  Every term of every sum is then a multiple of a known power of two g:

    forward          w_1 .. w_D v                 g = 2^-(2D + 4)
    table gradient   w_1 .. w_D go                g = 2^-2D
    input gradient   scale w_.. (D - 1 of them) go (v_1 - v_0)     g = 2^-(2(D - 1) + 4)

and while abs_sum / g < 2^24 (fp32; 2^11 for a half accumulator, with g >= 2^-24 and abs_sum <= 65504) every partial sum in ANY
order is exact: the kernel must equal the double-precision oracle bitwise, whatever the atomic order, the DPP scan or the
multiply-add contraction.  tests/test_hashgrid_instances_cpu.py proves these premises from the oracle's abs_sum for every case
the GPU tests run.
"""
import numpy as np
import torch

from tests.test_hashgrid_pairs_gpu import INSIDE_ROWS, _cells, _exact_grid, _probe_positions, _probe_table  # noqa: F401

DIMS = [2, 3, 4]
FEATURES = [1, 2, 4, 8]
LOG2_T = [8, 12]
COUNTS = [1, 65, 257, 1000]        # one lane, a wave and a lane, a workgroup and a lane, a ragged fourth workgroup
HALF_COUNTS = [1, 65, 257]         # the half-accumulator probe


def g_forward(D):
    return 2.0 ** -(2 * D + 4)


def g_params(D):
    return 2.0 ** -(2 * D)


def g_input(D):
    return 2.0 ** -(2 * (D - 1) + 4)


def table_seed(D, F, log2_T):
    return 1000 * D + 10 * F + log2_T


def probe_dout(n, L, F, seed, sparse=False):
    """Row-major [n, L*F] integer gradients.  Dense: |go| <= 2, every fourth row (i % 4 == 3) exactly zero.  Sparse (the half
    probe): go in {-1, 0, 1}, three rows of four (i % 4 != 0) exactly zero.  A zero row is zero on every level: the atomic
    kernel's `!any` skip."""
    g = torch.Generator().manual_seed(seed)
    lim = 1 if sparse else 2
    go = torch.randint(-lim, lim + 1, (n, L * F), generator=g).float()
    i = torch.arange(n)
    go[(i % 4 != 0) if sparse else (i % 4 == 3)] = 0.0
    return go


def level_major(dout_rm, L, F):
    """[n, L*F] -> contiguous [L, n, F]"""
    n = dout_rm.shape[0]
    return dout_rm.view(n, L, F).permute(1, 0, 2).contiguous()


def misread_as_level_major(dout_rm, L, F):
    """The row-major gradient a kernel sees when it reads the row-major buffer with level-major strides."""
    n = dout_rm.shape[0]
    return dout_rm.contiguous().view(L, n, F).permute(1, 0, 2).reshape(n, L * F).contiguous()


def exact_f32(ref64):
    """The double-precision oracle result as fp32, which it must be exactly."""
    ref64 = np.asarray(ref64, np.float64)
    r32 = ref64.astype(np.float32)
    assert np.array_equal(r32.astype(np.float64), ref64), "the oracle's result is no fp32 number: the probe is not exact"
    return r32


def assert_bits(got, ref64, what):
    """got (fp32 or fp16 tensor / array) is BITWISE the oracle's double result (which is an fp32 number)."""
    if isinstance(got, torch.Tensor):
        got = got.detach().float().cpu().numpy()
    got = np.ascontiguousarray(got, np.float32).reshape(-1)
    ref = exact_f32(ref64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = got.view(np.uint32) == ref.view(np.uint32)
    if not same.all():
        i = int(np.argmin(same))
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} values are not bitwise the oracle's; first at {i}: got {got[i]!r}, "
                             f"ref {ref[i]!r}")


RANDOM_N = 4099   # the sample count of the random-data bounds (tests/test_kernels_gpu.py::test_hashgrid_backward's)


def random_dout(meta, n, seed, loss_scaled=False):
    """Row-major [n, L*F] random gradients with exact-zero rows (5, and every 16th).  Standard normal, or -- what a loss scale of
    128 makes of them, for the half-gradient bound -- magnitudes uniform in [1, 10] with a random sign."""
    g = torch.Generator().manual_seed(seed)
    if loss_scaled:
        mag = 1.0 + 9.0 * torch.rand(n, meta.n_output_dims, generator=g)
        dout = mag * (torch.randint(0, 2, (n, meta.n_output_dims), generator=g).float() * 2.0 - 1.0)
    else:
        dout = torch.randn(n, meta.n_output_dims, generator=g)
    if n > 5:
        dout[5] = 0.0
    dout[15::16] = 0.0
    return dout


def level_slices(meta):
    """per level: slice of the flat parameter vector"""
    F = meta.n_features
    return [slice(int(meta.offset[l]) * F, (int(meta.offset[l]) + int(meta.size[l])) * F) for l in range(meta.n_levels)]
