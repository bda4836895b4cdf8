"""The radix-select kernels (csrc/select.hip) behind ``ops.order_statistics`` / ``quantile`` / ``weighted_percentile``, the automatic
colour ranges built on them (``flow_colours(max_radius="auto")``, ``depth_colours(lo="auto", hi="auto")``: the reference's ``None`` defaults) and the scene boxes of the
sources, on the GPU: bit for bit against the models of tests/_select_ref.py, and against the recording of the reference's own code
(tests/golden/select.npz, record_select.py) within the derived bounds that tests/test_select_cpu.py checks on the CPU."""
import os

import numpy as np
import pytest
import torch

from tests import _colour_ref as C
from tests import _frame_ref as R
from tests import _select_ref as S
from tests.golden import record_select as RS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")
QS = (0.0, 0.02, 0.5, 0.98, 0.99, 1.0)
EPS32 = float(np.finfo(np.float32).eps)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def unaligned(a):
    """The same values on the device at a base that is no multiple of 16 bytes (the scalar-load path)."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {int(np.argmin(ok))}: {got[~ok][:3]} vs {want[~ok][:3]}"


def probe_ranks(n):
    """0, n - 1 and both neighbours of the two ranks of every q."""
    r = {0, n - 1}
    for q in QS:
        lo, hi, _ = S.quantile_ranks(q, n)
        r |= {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1}
    return sorted(v for v in r if 0 <= v < n)


def check_flat(x, what, to_dev=dev):
    from emernerf_amd import ops
    t = to_dev(x)
    ranks = probe_ranks(x.size)
    assert_same_bits(ops.order_statistics(t, ranks).cpu().numpy(), S.order_statistics(x, ranks), what + ": order statistics")
    got = ops.quantile(t, list(QS))
    assert got.shape == (len(QS),) and got.dtype == torch.float32 and got.is_cuda
    assert_same_bits(got.cpu().numpy(), [S.quantile(x, q) for q in QS], what + ": quantile")


def check_columns(x, what, to_dev=dev):
    from emernerf_amd import ops
    t = to_dev(x)
    n, cols = x.shape
    ranks = probe_ranks(n)
    got = ops.order_statistics(t, ranks, dim=0)
    assert got.shape == (len(ranks), cols)
    assert_same_bits(got.cpu().numpy(), np.stack([S.order_statistics(x[:, c], ranks) for c in range(cols)], -1), what + ": order statistics")
    got = ops.quantile(t, list(QS), dim=0)
    assert got.shape == (len(QS), cols)
    assert_same_bits(got.cpu().numpy(), [[S.quantile(x[:, c], q) for c in range(cols)] for q in QS], what + ": quantile")


def keys_to_floats(keys):
    keys = np.asarray(keys, dtype=np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys)
    return bits.astype(np.uint32).view(np.float32)


# ----------------------------------------------------------------------------------------- order statistics and quantile
SLICE = 1024      # ops.SELECT_VECTOR_ROWS: rows of one workgroup step on the 16-byte-load path (256 on the scalar path)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 300001, SLICE * 1024 + 1])
def test_contiguous_sizes(hip_lib, n):
    """Every size around a lane group, a workgroup step of either path and the grid: 300 001 rows wrap the scalar path's grid
    (1024 workgroups x 256 rows), 1024 x 1024 + 1 the vector path's."""
    from emernerf_amd import ops
    assert SLICE == ops.SELECT_VECTOR_ROWS and ops.SELECT_MAX_BLOCKS == 1024
    rng = np.random.default_rng(3000 + n % 1000)
    x = (rng.standard_normal(n) * 50).astype(np.float32)
    check_flat(x, f"n={n}")
    if n <= 300001:
        check_flat(x, f"n={n} unaligned", unaligned)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 257, SLICE - 1, SLICE + 1, 300001])
def test_column_strided_sizes(hip_lib, n):
    """[n, 3] with dim=0: one read of the rows serves the three columns (16-byte loads), and the same from an unaligned base."""
    rng = np.random.default_rng(3100 + n % 1000)
    x = (rng.standard_normal((n, 3)) * np.array([30.0, 0.01, 1000.0])).astype(np.float32)
    check_columns(x, f"[{n}, 3]")
    if n <= SLICE + 1:
        check_columns(x, f"[{n}, 3] unaligned", unaligned)


def test_other_strides_and_dims(hip_lib):
    """Strides without a vector path (2, 5: more columns than one call takes), dim=None of a matrix, the last dim, a scalar q and
    rank, and a half-precision input (dtype follows x)."""
    from emernerf_amd import ops
    rng = np.random.default_rng(3200)
    for cols in (2, 5):
        check_columns((rng.standard_normal((777, cols)) * 7).astype(np.float32), f"[777, {cols}]")
    x = (rng.standard_normal((41, 6)) * 7).astype(np.float32)
    t = dev(x)
    assert_same_bits(ops.quantile(t, 0.3).cpu().numpy(), S.quantile(x, 0.3), "dim=None")
    assert ops.quantile(t, 0.3).shape == () and ops.order_statistics(t, 5).shape == ()
    got = ops.quantile(t, [0.3, 0.9], dim=1)
    assert got.shape == (2, 41)
    assert_same_bits(got.cpu().numpy(), [[S.quantile(x[r], q) for r in range(41)] for q in (0.3, 0.9)], "dim=1")
    assert_same_bits(ops.quantile(t, torch.tensor([0.3, 0.9]), dim=-1).cpu().numpy(), got.cpu().numpy(), "tensor q, dim=-1")
    h = t.half()
    got = ops.quantile(h, 0.5)
    assert got.dtype == torch.float16
    assert_same_bits(got.float().cpu().numpy(), np.float32(np.float16(S.quantile(h.float().cpu().numpy(), 0.5))), "half")
    for bad in (lambda: ops.quantile(t, 1.5), lambda: ops.order_statistics(t, 41 * 6), lambda: ops.order_statistics(t, 0.5),
                lambda: ops.quantile(t.double(), 0.5), lambda: ops.quantile(t.cpu(), 0.5), lambda: ops.quantile(t[:0], 0.5)):
        with pytest.raises(Exception):
            bad()


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_keys_that_differ_in_one_byte(hip_lib, byte):
    """All keys share three bytes: exactly one pass has more than one non-empty bin."""
    rng = np.random.default_rng(3300 + byte)
    base = np.uint32(0xC2A57331) & ~np.uint32(0xFF << (8 * byte))
    digits = rng.integers(0x30 if byte == 3 else 0, 0xD0 if byte == 3 else 256, 5000).astype(np.uint32)
    x = keys_to_floats(base | (digits << np.uint32(8 * byte)))
    assert np.isfinite(x).all() and len(np.unique(x)) > 100
    check_flat(x, f"byte {byte}")


def test_equal_keys_two_values_and_special_values(hip_lib):
    from emernerf_amd import ops
    check_flat(np.full(3001, -7.25, np.float32), "all equal")
    rng = np.random.default_rng(3400)
    check_flat(rng.choice(np.array([1.5, -2.0], np.float32), 3001), "two values")
    special = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 3.4e38, -3.4e38, 1.0, -1.0], np.float32)
    finite = special[np.isfinite(special)]
    x = np.concatenate([special, rng.choice(finite, 2000), (rng.standard_normal(2000) * 1e-3).astype(np.float32)])
    rng.shuffle(x)
    t = dev(x)
    ranks = list(range(0, x.size, 7)) + [x.size - 1]
    assert_same_bits(ops.order_statistics(t, ranks).cpu().numpy(), S.order_statistics(x, ranks), "special values")
    want = [S.quantile(x, q) for q in QS]               # q = 0 and 1 interpolate between infinities: NaN on both sides
    assert sum(np.isfinite(v) for v in want) >= 4
    assert_same_bits(ops.quantile(t, list(QS)).cpu().numpy(), want, "special values: quantile")
    zeros = dev(np.array([-0.0, 0.0, -0.0], np.float32))
    assert ops.order_statistics(zeros, [0, 1, 2]).cpu().numpy().tolist() == [0.0, 0.0, 0.0]


def test_one_nan_gives_nan(hip_lib):
    from emernerf_amd import ops
    rng = np.random.default_rng(3500)
    x = rng.standard_normal(5000).astype(np.float32)
    x[1234] = np.nan
    t = dev(x)
    assert torch.isnan(ops.quantile(t, list(QS))).all()
    ranks = [0, 2500, 4998, 4999]
    assert_same_bits(ops.order_statistics(t, ranks).cpu().numpy(), S.order_statistics(x, ranks), "NaN sorts last")
    cols = np.stack([x, np.ones_like(x), -np.abs(np.nan_to_num(x))], -1).astype(np.float32)     # the NaN marks its own column only
    got = ops.quantile(dev(cols), 0.5, dim=0).cpu().numpy()
    assert np.isnan(got[0]) and got[1] == 1.0
    assert_same_bits(got[2], S.quantile(cols[:, 2], 0.5), "a NaN in another column")


def test_more_jobs_than_one_launch_and_repeatability(hip_lib):
    """40 quantiles of three columns (240 ranks: 30 calls at 4 per column) equal the model; two runs give the same bits."""
    from emernerf_amd import ops
    rng = np.random.default_rng(3600)
    x = (rng.standard_normal((20011, 3)) * 20).astype(np.float32)
    qs = np.linspace(0, 1, 40).tolist()
    assert 2 * len(qs) > ops.SELECT_PER_SOURCE_MAX and 3 * len(qs) > ops.SELECT_JOBS_MAX
    t = dev(x)
    a = ops.quantile(t, qs, dim=0)
    assert_same_bits(a.cpu().numpy(), [[S.quantile(x[:, c], q) for c in range(3)] for q in qs], "40 quantiles")
    b = ops.quantile(t, qs, dim=0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    w = dev(rng.uniform(0, 1, 20011 * 3).astype(np.float32))
    p, q = ops.weighted_percentile(t, w, [0.5, 50, 99.5]), ops.weighted_percentile(t, w, [0.5, 50, 99.5])
    assert torch.equal(p.view(torch.int64), q.view(torch.int64))


# ------------------------------------------------------------------------------------------------------ weighted percentile
def assert_same_f64(got, want, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | ((got == 0) & (want == 0)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), f"{what}: {got} vs {want}"


PS = [0.0, 0.5, 2.0, 50.0, 73.3, 99.5, 100.0]


def test_weighted_percentile_equals_the_model(hip_lib):
    from emernerf_amd import ops
    rng = np.random.default_rng(3700)
    cases = {}
    for k in range(len(RS.DEPTH_SHAPES)):
        cases[f"image {k}"] = RS.depth_image(k)
    n = 70001                                                    # several workgroups; odd: a scalar tail on the vector path
    cases["large"] = (np.exp(rng.uniform(-3, 6, n)).astype(np.float32), np.clip(rng.uniform(-0.3, 1.3, n), 0, 1).astype(np.float32))
    x = rng.standard_normal(5001).astype(np.float32)
    w = rng.uniform(0, 1, 5001).astype(np.float32)
    w[np.argsort(x)[1000:3500]] = 0                              # a long run of zero weights in the middle of the order
    w[np.argsort(x)[:40]] = 0                                    # ... and at its start
    w[np.argsort(x)[-40:]] = 0                                   # ... and at its end
    cases["zero runs"] = (x, w)
    cases["ties"] = (rng.integers(-5, 6, 4000).astype(np.float32), rng.uniform(0, 1, 4000).astype(np.float32))
    cases["odd weights"] = (x, np.concatenate([np.array([np.nan, -1.0, 2.0, 1e-12, 1.0], np.float32), w[5:]]))
    for name, (x, w) in cases.items():
        want = S.weighted_percentile(x, w, PS)
        got = ops.weighted_percentile(dev(x), dev(w), PS)
        assert got.dtype == torch.float64 and got.shape == (len(PS),) and got.is_cuda
        assert_same_f64(got.cpu().numpy(), want, name)
        if x.size <= 5001:
            assert_same_f64(ops.weighted_percentile(unaligned(x), unaligned(w), PS).cpu().numpy(), want, name + " unaligned")
    x, w = cases["image 1"]
    assert ops.weighted_percentile(dev(x), dev(w), 50.0).shape == ()


def test_weighted_percentile_unit_and_zero_weights(hip_lib):
    """Weights all 1 give the unweighted bracket; a total of zero gives the largest value, as np.interp does."""
    from emernerf_amd import ops
    rng = np.random.default_rng(3800)
    x = rng.standard_normal(4099).astype(np.float32)
    t = dev(x)
    ones = ops.weighted_percentile(t, torch.ones_like(t), PS).cpu().numpy()
    assert_same_f64(ones, S.weighted_percentile(x, np.ones_like(x), PS), "weights 1")
    none = ops.weighted_percentile(t, None, PS).cpu().numpy()
    assert_same_f64(none, S.weighted_percentile(x, None, PS), "no weights")
    np.testing.assert_allclose(ones, none, rtol=1e-12, atol=1e-12)          # (t is rounded at another scale)
    s = np.sort(x).astype(np.float64)
    want = np.interp(np.array(PS) * (x.size / 100), np.arange(1, x.size + 1), s)      # the reference's formula in fp64
    np.testing.assert_allclose(none, want, rtol=1e-9, atol=1e-12)
    zero = ops.weighted_percentile(t, torch.zeros_like(t), [0.5, 99.5]).cpu().numpy()
    assert zero.tolist() == [float(x.max())] * 2


def test_recorded_percentiles_within_the_interval(hip_lib):
    """The device's percentiles of the recorded images lie, like the reference's own, in [M(t (1 - g)), M(t (1 + g))]."""
    from emernerf_amd import ops
    z = np.load(os.path.join(GOLDEN, "select.npz"))
    for k in range(len(RS.DEPTH_SHAPES)):
        depth, opacity = RS.depth_image(k)
        got = ops.weighted_percentile(dev(depth), dev(opacity), list(RS.PERCENTS)).cpu().numpy()
        for p, v, ref in zip(RS.PERCENTS, got, z[f"depth/{k}/percentiles"]):
            a, b = S.percentile_interval(depth, opacity, p)
            print(f"image {k} p {p}: device {v!r} reference {ref!r} interval [{a!r}, {b!r}]")
            assert a <= v <= b and a <= ref <= b


# -------------------------------------------------------------------------------------------------- automatic depth range
@pytest.mark.parametrize("k", [0, 1])
def test_depth_colours_with_automatic_bounds(hip_lib, k):
    from emernerf_amd import ops
    z = np.load(os.path.join(GOLDEN, "select.npz"))
    depth, opacity = RS.depth_image(k)
    d, o = dev(depth), dev(opacity)
    got = ops.depth_colours(d, o, "auto", "auto")
    assert got.dtype == torch.uint8 and tuple(got.shape) == depth.shape + (3,)
    lo_a, hi_a = ops.weighted_percentile(d, o, [0.5, 99.5]).tolist()
    assert torch.equal(got, ops.depth_colours(d, o, lo_a - EPS32, hi_a + EPS32))
    assert torch.equal(ops.depth_colours(d, o, "auto", 120.0), ops.depth_colours(d, o, lo_a - EPS32, 120.0))       # hi is kept
    assert torch.equal(ops.depth_colours(d, o, 4.0, "auto"), ops.depth_colours(d, o, 4.0, hi_a + EPS32))
    assert not torch.equal(got, ops.depth_colours(d, o))
    assert torch.equal(ops.compose_frame([("depth", 0, 0, d, o)], *depth.shape, 1, 1, False, "auto", "auto"), got)
    assert ops.depth_range("auto", "auto", d, o) == ops.depth_range(lo_a - EPS32, hi_a + EPS32)
    # against the recording: every pixel is a row its bounds' intervals allow; no more second choices than pixels that have one
    pairs = [S.percentile_interval(depth, opacity, p) for p in RS.PERCENTS]
    ok = RS.acceptable_rows(depth, opacity, pairs[0], pairs[1])
    table = R.table_with_black(z["turbo8"])
    g = got.cpu().numpy()
    hit = np.all(table[None, None] == g[:, :, None, :], axis=-1) & ok
    assert hit.any(-1).all(), f"{int((~hit.any(-1)).sum())} pixels outside their acceptable rows"
    second, ambiguous = int(np.any(g != z[f"depth/{k}/image8"], axis=-1).sum()), int((ok.sum(-1) > 1).sum())
    print(f"image {k}: {second} pixels differ from the recording, {ambiguous} have more than one acceptable row")
    assert second <= ambiguous


def test_depth_frames_with_several_depth_tiles_still_refuse(hip_lib):
    from emernerf_amd import ops
    depth, opacity = RS.depth_image(0)
    d, o = dev(depth), dev(opacity)
    H, W = depth.shape
    for kw in (dict(lo="auto"), dict(hi="auto")):
        with pytest.raises(NotImplementedError, match="one depth"):
            ops.compose_frame([("depth", 0, 0, d, o), ("depth", 0, 1, d, o)], H, W, 1, 2, False, **kw)
        with pytest.raises(NotImplementedError, match="one depth"):
            ops.compose_frame([("grey1", 0, 0, d, None)], H, W, 1, 1, False, **kw)
    rgb = torch.rand(H, W, 3, device=DEV)
    frame = ops.compose_frame([("colour3", 0, 0, rgb, None), ("depth", 1, 0, d, o)], H, W, 2, 1, True, "auto", "auto")
    assert torch.equal(frame[H:], ops.compose_frame([("depth", 0, 0, d, o)], H, W, 1, 1, True, "auto", "auto"))


# ------------------------------------------------------------------------------------------------- automatic flow radius
@pytest.mark.parametrize("name", ["batch", "zero"])
def test_flow_colours_with_automatic_radius(hip_lib, name):
    from emernerf_amd import ops
    z = np.load(os.path.join(GOLDEN, "select.npz"))
    flow = z[f"flow/{name}/flow"]
    f = dev(flow)
    r = ops.quantile(f, 0.99, radius=True)
    assert r.shape == () and r.dtype == torch.float32
    rec = float(z[f"flow/{name}/radius"])
    radius = np.hypot(flow[:, 0].astype(np.float64), flow[:, 1].astype(np.float64)).astype(np.float32)
    lo, hi, _ = S.quantile_ranks(0.99, radius.size)
    a, b = S.order_statistics(radius, [lo, hi])
    bound = S.quantile_bound(a, b) + float(S.ulp(max(a, b)))            # hypotf against torch's complex abs: one more ulp
    print(f"{name}: radius {float(r)!r}, recorded {rec!r}, bound {bound:.3e}")
    assert abs(float(r) - rec) <= bound
    delta = abs(float(r) - rec) / rec if rec > 0 else 0.0
    wheel = ops.colour_wheel()
    for bg in ("bright", "dark"):
        got = ops.flow_colours(f, "auto", bg)
        assert torch.equal(got, ops.flow_colours(f, float(r), bg))
        C.assert_within(got.cpu().numpy(), z[f"flow/{name}/rgb/{bg}"].astype(np.float64), C.FLOW_BOUND + delta * (1 + delta),
                        f"{name} flow colours vs the recording, {bg}")
    if name == "zero":
        assert float(r) == 0.0          # no division: the colours of radius 0, not NaN
        assert torch.equal(ops.flow_colours(f, "auto", "bright"), torch.ones_like(f))
    a2, b2 = ops.flow_colours_multi([f, -f], "auto", "dark")
    assert torch.equal(a2, ops.flow_colours(f, "auto", "dark")) and torch.equal(b2, ops.flow_colours(-f, "auto", "dark"))
    img = f[: (flow.shape[0] // 4) * 4].reshape(4, -1, 3)
    assert ops.flow_colours(img, "auto").shape == img.shape


# -------------------------------------------------------------------------------------------------------------- scene boxes
def test_lidar_and_camera_boxes(hip_lib):
    from emernerf_amd.lidar_source import LidarSource
    from emernerf_amd.pixel_source import PixelSource
    z = np.load(os.path.join(GOLDEN, "select.npz"))
    n, f, p = RS.LIDAR["n"], RS.LIDAR["factor"], RS.LIDAR["percentile"]
    for case in ("round", "flat"):
        o, d, r = RS.lidar_points(case)
        src = LidarSource(o.to(DEV), d.to(DEV), r.to(DEV), torch.zeros(n, dtype=torch.int64, device=DEV), seed=5)
        subset = torch.from_numpy(z[f"lidar/{case}/subset"])
        box = src.get_aabb(f, p, subset=subset.to(DEV))
        assert box.shape == (6,) and box.dtype == torch.float32 and box.is_cuda
        pts = (o + d * r)[subset].numpy()
        got, want = box.cpu().numpy(), z[f"lidar/{case}/aabb"]
        for j, q in enumerate((p, 1 - p)):
            for c in range(3):
                lo, hi, _ = S.quantile_ranks(q, pts.shape[0])
                a, b = S.order_statistics(pts[:, c], [lo, hi])
                # (the points themselves: a product and a sum, rounded as torch rounds them on either device)
                assert abs(float(got[3 * j + c]) - float(want[3 * j + c])) <= S.quantile_bound(a, b), (case, j, c, got, want)
        assert (got[5] == 20.0) == (case == "flat")
        a1, a2 = src.get_aabb(f, p), src.get_aabb(f, p)
        assert torch.equal(a1, a2)                                                  # deterministic for a seed ...
        other = LidarSource(o.to(DEV), d.to(DEV), r.to(DEV), torch.zeros(n, dtype=torch.int64, device=DEV), seed=6).get_aabb(f, p)
        assert not torch.equal(a1, other)                                           # ... which the draw depends on
        g = torch.Generator(device=DEV).manual_seed(5)                              # int(n / f) points of a seeded device randperm
        idx = torch.randperm(n, generator=g, device=DEV)[: int(n / f)]
        assert idx.numel() == 1000 and torch.equal(a1, src.get_aabb(f, p, subset=idx))
    for cams in RS.CAMS:
        c2w = RS.camera_poses(cams).to(DEV)
        m = c2w.shape[0]
        src = PixelSource(torch.zeros(m, 2, 2, 3, device=DEV), c2w, torch.eye(3, device=DEV).repeat(m, 1, 1),
                          cam_ids=(torch.arange(m, device=DEV) % cams))
        box = src.get_aabb()
        assert box.is_cuda and box.dtype == torch.float32
        np.testing.assert_array_equal(box.cpu().numpy(), z[f"pixel/{cams}/aabb"])
        np.testing.assert_array_equal(src.get_aabb(num_cams=cams).cpu().numpy(), z[f"pixel/{cams}/aabb"])
    with pytest.raises(ValueError):
        src.get_aabb(num_cams=4)
