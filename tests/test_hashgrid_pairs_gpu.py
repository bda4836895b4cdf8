"""The x-pair path of hashgrid_fwd_kernel (hashed power-of-two levels): exact probes, random tables, slice bitmaps, fp16 tables.

Small grids whose hashed power-of-two levels start at low resolution, so that a few hundred samples reach every case of the pair
path: even and odd x cells in one wave, idx0 odd under an even x (the aligned entry pair arrives swapped), x in the last cell of a
level and beyond it (`gi[0] >= res` switches the one-bit-per-pair bitmap rule off for the whole wave), coordinates of exactly 0 and 1.

Exact probes.  Per-level scale 2 with base 4 makes every level's scale an integer (3, 7, 15, 31, 63), so positions that are multiples
of 1/4 give interpolation weights that are multiples of 1/4; with table entries that are small integers times 2^-4 every product
(a multiple of 2^-10, at most 1/2) and every partial sum (at most 4) is exact in fp32.  The kernel must then equal the oracle BITWISE
whatever the compiler contracts into multiply-adds.  test_exact_probe_covers_the_pair_cases checks on the CPU that the probe is what
this paragraph says."""
import numpy as np
import pytest
import torch

from tests._bounds import assert_bound, c_forward, sliced_plan
from tests.test_kernels_gpu import _dev, _inputs

COUNTS = [1, 63, 65, 257, 1000]   # one lane, wave tails, a ragged last workgroup
FEATURES = [1, 2, 4]
LOG2_T = [8, 12]
PRIMES = (1, 2654435761, 805459861, 3674653429)   # the coherent-prime hash of the reference's grid encoding
INSIDE_ROWS = 128   # the first two waves hold no x beyond the level (the one-bit-per-pair rule stays on), later waves do
# absolute tolerance of tests/test_kernels_gpu.py::test_hashgrid_fwd (a literal there; the per-entry bound and its constant are imported)
FWD_ATOL = 2e-6


def _exact_grid(oracle, F, log2_T, D=3):
    """base 4 -> 64 in five levels of integer scale; level 1 (res 8) is the first hashed one at T = 2^8, level 3 (res 32) at T = 2^12"""
    from emernerf_amd import _lib
    meta = oracle.grid_meta(D, 5, F, log2_T, 4, 2.0)
    return meta, _lib.make_grid_desc(D, 5, F, log2_T, 4, 2.0)


def _random_grid(oracle, F, log2_T):
    """base 4 -> 64 in four levels (scales that are no integers)"""
    from emernerf_amd import _lib
    meta = oracle.grid_meta_from_encoder_args(3, 4, 4, 64, log2_T, F)
    return meta, _lib.make_grid_desc(3, 4, F, log2_T, 4, meta.per_level_scale)


def _probe_positions(n, D=3):
    """Row i: multiples of 1/4, x fastest.  x runs over 0 .. 1 in the first INSIDE_ROWS rows and over 0 .. 1.5 (beyond the level) after
    them; the other coordinates over 0 .. 1.5 throughout."""
    i = np.arange(n)
    inside = i < INSIDE_ROWS
    jx = np.where(inside, i % 5, i % 7)
    rest = np.where(inside, i // 5, i // 7)
    cols = [jx]
    for _ in range(1, D):
        cols.append(rest % 7)
        rest = rest // 7
    return torch.tensor(np.stack(cols, 1) / 4.0, dtype=torch.float32)


def _probe_table(meta, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (meta.n_params,), generator=g).float() / 16.0


def _cells(meta, x, level):
    """(gi [N, D] int64, w [N, D] float32) of cell_of: pos = fmaf(scale, x, 0.5) -- exact here, see the asserts of the caller"""
    pos = np.float64(meta.scale[level]) * x.numpy().astype(np.float64) + 0.5
    fl = np.floor(pos)
    return fl.astype(np.int64), (pos - fl).astype(np.float32), pos


def _pair_levels(meta):
    return [l for l in range(meta.n_levels) if meta.hashed[l] and (int(meta.size[l]) & (int(meta.size[l]) - 1)) == 0]


@pytest.mark.parametrize("log2_T", LOG2_T)
def test_exact_probe_covers_the_pair_cases(oracle, log2_T):
    meta, _ = _exact_grid(oracle, 2, log2_T)
    assert np.array_equal(meta.scale, np.array([3, 7, 15, 31, 63], np.float32)) and np.array_equal(meta.res, [4, 8, 16, 32, 64])
    levels = _pair_levels(meta)
    assert levels and levels[0] == (1 if log2_T == 8 else 3), (levels, meta.hashed, meta.size)
    n = max(COUNTS)
    x = _probe_positions(n)
    assert set(np.unique(x.numpy())) >= {0.0, 1.0}
    for l in levels:
        gi, w, pos = _cells(meta, x, l)
        assert np.array_equal(pos, pos.astype(np.float32)) and np.array_equal(w * 4, np.round(w * 4)), "weights are no multiples of 1/4"
        res, mask = int(meta.res[l]), int(meta.size[l]) - 1
        x_even = gi[:, 0] % 2 == 0
        for wave in range(0, n - 63, 64):   # every full wave mixes even and odd x cells
            assert 0 < x_even[wave:wave + 64].sum() < 64
        beyond = gi[:, 0] >= res
        assert not beyond[:INSIDE_ROWS].any() and beyond[INSIDE_ROWS:257].any(), "x beyond the level: none in the first waves, some later"
        assert (gi[:, 0] == res - 1).any(), "x in the last cell of the level"
        swapped = False
        for m in range(4):
            h = ((gi[:, 1] + (m & 1)) * PRIMES[1]) ^ ((gi[:, 2] + (m >> 1)) * PRIMES[2])
            idx0 = (gi[:, 0] ^ h) & mask
            swapped |= bool((x_even & (idx0 % 2 == 1)).any()) and bool((x_even & (idx0 % 2 == 0)).any())
        assert swapped, "idx0 odd with x even (and idx0 even with x even)"


def _forward(desc, x, p, want_masks=False):
    from emernerf_amd import ops
    return ops.hashgrid_fwd_raw(desc, x, p, level_major=False, want_masks=want_masks)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("log2_T", LOG2_T)
@pytest.mark.parametrize("F", FEATURES)
def test_exact_probes_equal_the_oracle_bitwise(hip_lib, oracle, F, log2_T, n):
    """fp32 table and its fp16 copy (the entries are fp16 numbers); row-major, level-major and the Jacobian forward's encoding"""
    from emernerf_amd import ops
    meta, desc = _exact_grid(oracle, F, log2_T)
    x, p = _probe_positions(n), _probe_table(meta, 10 * F + log2_T)
    assert torch.equal(p.half().float(), p)
    ref = oracle.hashgrid_fwd(meta, x, p)
    dev = _dev()
    xd, pd = x.to(dev), p.to(dev)
    for tag, table in (("fp32", pd), ("fp16", pd.half())):
        out = _forward(desc, xd, table)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"{tag} table: not bitwise the oracle's"
        lm = ops.hashgrid_fwd_raw(desc, xd, table, level_major=True)
        assert torch.equal(lm.permute(1, 0, 2).reshape(n, -1), out), f"{tag} table: level-major differs from row-major"
    enc_jac, _ = ops.hashgrid_fwd_raw(desc, xd, pd, level_major=False, jac_row0=0)
    assert np.array_equal(enc_jac.cpu().numpy().view(np.uint32), ref.view(np.uint32)), "Jacobian forward: not bitwise the oracle's"


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("log2_T", LOG2_T)
@pytest.mark.parametrize("F", FEATURES)
def test_random_tables_within_the_forward_bounds(hip_lib, oracle, F, log2_T, n):
    """tcnn-style init U(-1e-4, 1e-4) and U(-0.3, 0.3) tables, fp32 and fp16-rounded, on random positions with the edge rows of
    tests/test_kernels_gpu._inputs: the tolerance and the per-entry bound of test_hashgrid_fwd"""
    meta, desc = _random_grid(oracle, F, log2_T)
    assert _pair_levels(meta), "no hashed power-of-two level"
    x, u = _inputs(meta, n, 100 * F + log2_T + n)   # u: U(-0.5, 0.5)
    dev = _dev()
    for name, p in (("tcnn init", u * 2e-4), ("U(-0.3, 0.3)", u * 0.6)):
        for tag, table in (("fp32", p), ("fp16", p.half())):
            ref = oracle.hashgrid_fwd(meta, x, table.float())
            ref64, fabs_ = oracle.hashgrid_fwd_bound(meta, x, table.float())
            out = _forward(desc, x.to(dev), table.to(dev)).cpu().numpy()
            np.testing.assert_allclose(out, ref, rtol=0, atol=FWD_ATOL)
            assert_bound(out, ref64, fabs_, c_forward(meta.n_dims), f"fwd pairs {name} {tag} F={F} T=2^{log2_T} n={n}", meta=meta, kind="fwd")


def _written_rows(masks, desc, n):
    """the bitmap words of the rows that exist, level by level (rows past a level's slice count are never written)"""
    from emernerf_amd import ops
    L = desc.n_levels
    n_words = (n + 63) // 64
    rows = (ops.mask_words(desc, n) - ops.MASK_SCRATCH) // (L * n_words)
    n_slices, _ = sliced_plan(desc, L)
    assert n_slices.max() <= rows, "a bitmap row shared by several slices: not what this helper reads"
    m = masks[:L * rows * n_words].reshape(L, rows, n_words)
    return rows, [m[l, :int(n_slices[l])] for l in range(L)]


def _check_bitmaps(desc, x, p, want_rows):
    from emernerf_amd import ops
    n = x.shape[0]
    plain = _forward(desc, x, p)
    enc, masks = _forward(desc, x, p, want_masks=True)
    assert torch.equal(enc, plain), "the encoding changes when bitmaps are requested"
    rows, got = _written_rows(masks, desc, n)
    assert rows == want_rows
    _, ref = _written_rows(ops.slice_masks(desc, x), desc, n)
    for l, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a, b), f"level {l}: the forward's bitmaps differ from emer_hashgrid_slice_masks"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("log2_T", LOG2_T)
@pytest.mark.parametrize("F", FEATURES)
def test_bitmaps_of_the_probes_64_rows(hip_lib, oracle, F, log2_T, n):
    """mask_q == 1, on the probe positions (the one-bit-per-pair rule on in the first waves and off behind them); fp32 and fp16 tables"""
    meta, desc = _exact_grid(oracle, F, log2_T)
    dev = _dev()
    x, p = _probe_positions(n).to(dev), _probe_table(meta, 3).to(dev)
    got = _check_bitmaps(desc, x, p, 64)
    half = _check_bitmaps(desc, x, p.half(), 64)
    assert all(torch.equal(a, b) for a, b in zip(got, half))
    if n >= 64:
        assert all(bool(g.any()) for g in got)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("F,log2_T", [(1, 21), (2, 20), (4, 19)])
def test_bitmaps_256_rows(hip_lib, oracle, F, log2_T, n):
    """mask_q == 4 (128 slices per level): two hashed levels of resolution 256 and 512, random positions with the edge rows"""
    from emernerf_amd import _lib
    meta = oracle.grid_meta(3, 2, F, log2_T, 256, 2.0)
    desc = _lib.make_grid_desc(3, 2, F, log2_T, 256, 2.0)
    assert _pair_levels(meta) == [0, 1]
    x, p = _inputs(meta, n, 5)
    x[-1, 0] = 1.25   # beyond the level
    dev = _dev()
    _check_bitmaps(desc, x.to(dev), p.to(dev), 256)
