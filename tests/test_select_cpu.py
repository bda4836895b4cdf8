"""The models of tests/_select_ref.py against torch and against the recording of the reference (tests/golden/select.npz,
record_select.py), without a GPU: the yardsticks that tests/test_select_gpu.py holds the radix-select kernels to."""
import os

import numpy as np
import pytest
import torch

from tests import _select_ref as S
from tests.golden import record_select as RS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QS = (0.0, 0.02, 0.5, 0.98, 0.99, 1.0)


def load():
    return np.load(os.path.join(GOLDEN, "select.npz"))


def seeded_arrays():
    rng = np.random.default_rng(2200)
    for n in (1, 2, 3, 7, 100, 255, 256, 257, 1000, 4001):
        yield rng.standard_normal(n).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4))
        yield np.exp(rng.uniform(-20, 20, n)).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), n)
        yield rng.integers(-3, 4, n).astype(np.float32)              # ties


def test_order_statistics_of_torch_quantile_equal_the_model():
    """With ``interpolation="lower"`` / ``"higher"`` torch.quantile returns the two order statistics it interpolates between: they
    must be the model's, bit for bit, for every q."""
    for x in seeded_arrays():
        t = torch.from_numpy(x)
        for q in QS:
            lo, hi, _ = S.quantile_ranks(q, x.size)
            a, b = S.order_statistics(x, [lo, hi])
            assert torch.quantile(t, q, interpolation="lower").numpy() == a, (x.size, q)
            assert torch.quantile(t, q, interpolation="higher").numpy() == b, (x.size, q)


def test_quantile_model_within_two_ulp_of_torch():
    """The interpolated value: the fused and the unfused lerp both lie within 2 ulp of max(|a|, |b|) of torch.quantile (derived: the
    unfused form rounds a product bounded by 2 max and then a sum; torch's CPU kernel may take either form)."""
    worst = 0.0
    for x in seeded_arrays():
        t = torch.from_numpy(x)
        for q in QS + (0.25, 0.731):
            want = float(torch.quantile(t, q))
            lo, hi, _ = S.quantile_ranks(q, x.size)
            a, b = S.order_statistics(x, [lo, hi])
            bound = S.quantile_bound(a, b)
            for fused in (True, False):
                got = float(S.quantile(x, q, fused))
                assert abs(got - want) <= bound, (x.size, q, fused, got, want, bound)
                worst = max(worst, abs(got - want) / bound)
    assert worst <= 1.0
    x = np.array([1.0, np.nan, 3.0], np.float32)
    assert np.isnan(S.quantile(x, 0.5)) and np.isnan(float(torch.quantile(torch.from_numpy(x), 0.5)))


def test_weighted_percentile_model_on_small_cases():
    """Hand-checked brackets: distinct values are np.interp over the exact cumulative weights; zero weights extend a plateau; a
    total of zero gives the largest value; ties merge into one node."""
    x = np.array([3.0, 1.0, 2.0, 4.0], np.float32)
    w = np.array([0.5, 0.25, 0.25, 1.0], np.float32)
    got = S.weighted_percentile(x, w, [0, 10, 12.5, 25, 50, 100])
    want = np.interp(np.array([0, 10, 12.5, 25, 50, 100]) * (2.0 / 100), np.cumsum(w[np.argsort(x)].astype(np.float64)), np.sort(x).astype(np.float64))
    np.testing.assert_allclose(got, want, rtol=1e-12)      # (t = p * (total / 100) is rounded twice: not np.interp's bits)
    z = S.weighted_percentile(np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([1.0, 0.0, 0.0, 1.0], np.float32), [60, 75])
    np.testing.assert_allclose(z, [3.2, 3.5], rtol=1e-12)   # t = 1.2 and 1.5: the plateau ends at 3, the last value that weighs nothing
    z = S.weighted_percentile(np.array([1.0, 2.0, 3.0, 4.0], np.float32), np.array([1.0, 0.0, 0.0, 1.0], np.float32), [25])
    assert z[0] == 1.0                                      # below the first node's weight: the left clamp
    assert S.weighted_percentile(np.array([5.0, 7.0, 6.0], np.float32), np.zeros(3, np.float32), [0.5, 99.5]).tolist() == [7.0, 7.0]
    tie = S.weighted_percentile(np.array([1.0, 2.0, 2.0, 2.0, 3.0], np.float32), np.ones(5, np.float32), [50])
    np.testing.assert_allclose(tie, [1.5], rtol=1e-12)      # nodes 1 | 2 (weight 3) | 3: t = 2.5 lies half way up the node of the twos


def test_recorded_percentiles_lie_in_the_model_interval():
    """The reference's own ``weighted_percentile`` (fp32 cumsum in argsort order) lies in [M(t (1 - g)), M(t (1 + g))]."""
    z = load()
    for k in range(len(RS.DEPTH_SHAPES)):
        depth, opacity = RS.depth_image(k)
        np.testing.assert_array_equal(depth, z[f"depth/{k}/depth"])
        np.testing.assert_array_equal(opacity, z[f"depth/{k}/opacity"])
        assert 0.15 < np.mean(opacity == 0) < 0.25
        for p, v in zip(RS.PERCENTS, z[f"depth/{k}/percentiles"]):
            a, b = S.percentile_interval(depth, opacity, p)
            assert a <= v <= b, (k, p, a, v, b)
            m = S.weighted_percentile(depth, opacity, [p])[0]
            assert a <= m <= b
            print(f"image {k} p {p}: reference {v!r} model {m!r} interval [{a!r}, {b!r}]")


def test_recorded_depth_image_rows_are_acceptable():
    """Every pixel of the recorded ``visualize_depth(lo=None, hi=None)`` image is one of the rows its bound intervals allow."""
    z = load()
    lut = z["turbo8"]
    for k in range(len(RS.DEPTH_SHAPES)):
        depth, opacity = RS.depth_image(k)
        pairs = [S.percentile_interval(depth, opacity, p) for p in RS.PERCENTS]
        ok = RS.acceptable_rows(depth, opacity, pairs[0], pairs[1])
        from tests import _frame_ref as R
        table = R.table_with_black(lut)
        hit = np.all(table[None, None] == z[f"depth/{k}/image8"][:, :, None, :], axis=-1) & ok
        assert hit.any(-1).all()
        assert np.sum(ok.sum(-1) > 1) <= (0.01 if k == 0 else 0.03) * depth.size


def test_recorded_flow_radius_and_boxes_follow_the_model():
    """The recorded radius quantile and lidar boxes against the quantile model on the recorded inputs (2 ulp bound; the radius one
    more for hypot against torch's complex abs), the camera boxes against the restated rule."""
    z = load()
    for name in ("batch", "zero"):
        flow = z[f"flow/{name}/flow"]
        r = np.hypot(flow[:, 0], flow[:, 1]).astype(np.float32)
        lo, hi, _ = S.quantile_ranks(0.99, r.size)
        a, b = S.order_statistics(r, [lo, hi])
        assert abs(float(S.quantile(r, 0.99)) - float(z[f"flow/{name}/radius"])) <= S.quantile_bound(a, b) + float(S.ulp(max(a, b)))
    assert float(z["flow/zero/radius"]) == 0.0
    for case in ("round", "flat"):
        o, d, r = RS.lidar_points(case)
        pts = (o + d * r)[torch.from_numpy(z[f"lidar/{case}/subset"])].numpy()
        assert pts.shape == (int(RS.LIDAR["n"] / RS.LIDAR["factor"]), 3)
        for c in range(3):
            for j, q in enumerate((RS.LIDAR["percentile"], 1 - RS.LIDAR["percentile"])):
                lo, hi, _ = S.quantile_ranks(q, pts.shape[0])
                a, b = S.order_statistics(pts[:, c], [lo, hi])
                want = float(z[f"lidar/{case}/aabb"][3 * j + c])
                got = float(S.quantile(pts[:, c], q))
                if j == 1 and c == 2 and case == "flat":
                    assert got < 20 and want == 20.0
                else:
                    assert abs(got - want) <= S.quantile_bound(a, b), (case, c, j, got, want)
    for cams in RS.CAMS:
        pos = RS.camera_poses(cams)[{1: 0, 3: 1, 5: 2, 6: 2}[cams]::cams, :3, 3].numpy()
        lo, hi = pos.min(0), pos.max(0)
        want = np.array([lo[0] - 40, lo[1] - 40, max(lo[2] - 5, -5), hi[0] + 40, hi[1] + 40, min(hi[2] + 20, 20)], np.float32)
        np.testing.assert_array_equal(z[f"pixel/{cams}/aabb"], want)
    tops = {cams: float(z[f"pixel/{cams}/aabb"][5]) for cams in RS.CAMS}
    assert tops[1] == 20.0 and tops[3] < 20.0 and float(z["pixel/3/aabb"][2]) == -5.0 and float(z["pixel/1/aabb"][2]) > -5.0


def test_host_side_refusals_and_limits():
    """What needs no GPU: the loader binds the new entries, a bound of None still raises and "auto" needs the image."""
    from emernerf_amd import _lib, ops
    assert "emer_select" in _lib.SIGNATURES and "emer_select_workspace_bytes" in _lib.INT64_FUNCTIONS
    assert ops.SELECT_PER_SOURCE_MAX == 4 and ops.SELECT_SOURCES_MAX == 4 and ops.SELECT_JOBS_MAX == 16
    with pytest.raises(NotImplementedError, match="percentile"):
        ops.depth_range(None, 120.0)
    with pytest.raises(ValueError, match="depth and opacity"):      # "auto" is the image's own range: it needs the image
        ops.depth_range("auto", 120.0)
    assert ops.AUTO == "auto"
    assert ops.depth_range(4.0, 120.0) == ops.depth_range()
