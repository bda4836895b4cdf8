"""The evaluation-colour kernels (csrc/colours.hip) and the eval loop's ``visualize`` output against recordings of the
reference (tests/golden/flow_colours.npz, feature_colours.npz; record_colours.py) and the float64 restatements and derived
bounds of tests/_colour_ref.py."""
import os
import types

import numpy as np
import pytest
import torch

from tests import _colour_ref as C
from tests.golden import make_golden as G
from tests.golden import record_colours as RC
from tests.test_colours_cpu import expected_feature_lists, load_feature_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------------------------------------------- flow colour wheel
def test_flow_colours_match_recording_and_restatement(hip_lib):
    from emernerf_amd import ops
    z = np.load(os.path.join(GOLDEN, "flow_colours.npz"))
    flow = dev(z["flow"])
    for bg in ("bright", "dark"):
        got = host(ops.flow_colours(flow, 1.0, bg))
        assert got.shape == z["flow"].shape and got.dtype == np.float32
        C.assert_within(got, z["rgb/" + bg].astype(np.float64), C.FLOW_BOUND, "flow colours vs the recording, " + bg)
        C.assert_within(got, C.flow_colours(z["flow"], z["WHEEL"], 1.0, bg), C.FLOW_BOUND, "flow colours vs float64, " + bg)
    # another radius, an image-shaped input, and both directions in one launch == two launches
    img = flow[:210].reshape(10, 21, 3)
    got = ops.flow_colours(img, 0.5, "dark")
    assert got.shape == (10, 21, 3)
    C.assert_within(host(got).reshape(-1, 3), C.flow_colours(z["flow"][:210], z["WHEEL"], 0.5, "dark"), C.FLOW_BOUND, "radius 0.5")
    a, b = ops.flow_colours_multi([flow, -flow], 1.0, "bright")
    assert torch.equal(a, ops.flow_colours(flow)) and torch.equal(b, ops.flow_colours(-flow))
    with pytest.raises(NotImplementedError):
        ops.flow_colours(flow, None)
    with pytest.raises(NotImplementedError):
        ops.flow_colours(flow, max_radius=None, background="dark")
    with pytest.raises(ValueError):
        ops.flow_colours(flow, 1.0, "grey")


def test_flow_colours_edge_rows_and_many_blocks(hip_lib):
    """Rows on wheel nodes and at radius 1 +- one ulp, tiled past one workgroup per member, vs the restatement; non-finite
    flows stay inside the wheel (no fault) and give a non-finite or clamped colour, never garbage rows elsewhere."""
    from emernerf_amd import ops
    w = ops.colour_wheel()
    one = np.float32(1.0)
    edge = [(0, 0, 0), (1, 0, 0), (np.nextafter(one, 0), 0, 0), (np.nextafter(one, 2), 0, 0), (0, 1, 0), (0, -1, 0), (-1, 0, 0),
            (-1, -1e-30, 0), (1, -1e-30, 0), (1e-30, 1e-30, 0), (3e38, 3e38, 0), (5, 0, 0), (0, -5, 0)]
    rng = np.random.default_rng(11)
    flow = np.concatenate([np.array(edge, dtype=np.float32), rng.standard_normal((4097 - len(edge), 3)).astype(np.float32)])
    for bg in ("bright", "dark"):
        got = host(ops.flow_colours(dev(flow), 1.0, bg))
        C.assert_within(got, C.flow_colours(flow, w, 1.0, bg), C.FLOW_BOUND, "edge rows, " + bg)
    bad = flow[:64].copy()
    bad[3] = (np.nan, 1.0, 0.0)
    bad[7] = (np.inf, -np.inf, 0.0)
    got = host(ops.flow_colours(dev(bad)))
    keep = np.ones(64, bool)
    keep[[3, 7]] = False
    np.testing.assert_array_equal(got[keep], host(ops.flow_colours(dev(flow[:64])))[keep])


# ------------------------------------------------------------------------------------------------------- feature colours
def _ops_lists(z, tag, i, features):
    from emernerf_amd import ops

    def colour(feat, pca, scale):
        return ops.feature_colours(dev(feat), *(dev(p) for p in pca), None if scale is None else dev(scale))

    def blend(a, o, b):
        return ops.blend_over(a if isinstance(a, torch.Tensor) else dev(a), dev(o), b if isinstance(b, torch.Tensor) else dev(b))
    return expected_feature_lists(z, tag, i, features, colour, blend)


@pytest.mark.parametrize("pe", [1, 0])
def test_feature_colours_and_blends_match_recording(hip_lib, pe):
    """E = 64, the reference's inputs, matrices and outputs: every list of the branch within the bound of the float64
    restatement (which the recording meets too: tests/test_colours_cpu.py), hence within twice the bound of the recording."""
    z, tag, images = load_feature_case(pe)
    for i, d in enumerate(images):
        rec = lambda k: z[f"{tag}res/{k}/{i}"]  # noqa: E731
        feats = d["features"].numpy()
        got = _ops_lists(z, tag, i, feats)
        ref = expected_feature_lists(z, tag, i, feats, lambda f, p, s: C.feature_colours(f, *p, s), C.blend_over, lists=rec)
        assert len(got) == (8 if pe else 6)
        for name, (want, bound) in ref.items():
            g = host(got[name])
            assert g.shape == rec(name).shape and g.dtype == np.float32
            if name.startswith("dynamic_") and "_on_" in name:
                # the blend's inputs on this side are this side's colours: carry their bound through the blend
                src = "static_dino_feats" if name == "dynamic_rgb_on_static_dinos" else "dynamic_dino_feats"
                o = z[f"{tag}raw/{i}/dynamic_opacity"].reshape(-1, 1).astype(np.float64)
                carried = 2 * ref[src][1] * (np.abs(1 - o) if name == "dynamic_rgb_on_static_dinos" else np.abs(o))
                bound = bound + carried          # |ours - recorded| input difference <= 2 x the colour bound
            C.assert_within(g.reshape(want.shape), want, bound, f"{tag}{name}[{i}] vs float64")
            err = np.abs(g.reshape(want.shape).astype(np.float64) - rec(name).reshape(want.shape))
            assert (err <= 2 * bound).all(), f"{tag}{name}[{i}] vs the recording"


def _random_case(N, E, seed):
    rng = np.random.default_rng(seed)
    feat = (rng.standard_normal((N, E)) * 0.5 + 0.2).astype(np.float32)
    mat = (rng.standard_normal((E, 3)) / np.sqrt(E)).astype(np.float32)
    p = feat.astype(np.float64) @ mat.astype(np.float64)
    lo = np.quantile(p, 0.2, axis=0).astype(np.float32) if N > 4 else (p.min(0) - 0.3).astype(np.float32)
    hi = np.quantile(p, 0.8, axis=0).astype(np.float32) if N > 4 else (p.max(0) + 0.3).astype(np.float32)
    scale = rng.random(N).astype(np.float32)
    return feat, mat, lo, hi, scale


@pytest.mark.parametrize("E", [3, 64, 384, 768])
def test_feature_colours_vs_float64_on_random_inputs(hip_lib, E):
    """Every group width (1, 16 and 64 lanes per row), one to three quads per lane, the scalar path (E = 3), rows that do not
    fill a workgroup and rows past one, with and without the per-row scale."""
    from emernerf_amd import ops
    for N in (1, 63, 65, 4097):
        feat, mat, lo, hi, scale = _random_case(N, E, 100 * E + N)
        for s in (None, scale):
            got = host(ops.feature_colours(dev(feat), dev(mat), dev(lo), dev(hi), None if s is None else dev(s)))
            ref, bound = C.feature_colours(feat, mat, lo, hi, s)
            assert got.shape == (N, 3)
            if N > 4:
                assert ((ref > 0) & (ref < 1)).any() and (ref == 0).any()      # both sides of the clamp are exercised
            C.assert_within(got, ref, bound, f"E={E} N={N} scale={s is not None}")


def test_feature_colours_degenerate_range_inf_and_nan(hip_lib):
    """One channel with hi == lo: +-inf clamps to 1 / 0, the 0 / 0 rows are NaN exactly where the restatement has NaN; NaN and
    inf FEATURES propagate as in torch (NaN stays NaN through the clamp)."""
    from emernerf_amd import ops
    feat, mat, lo, hi, scale = _random_case(257, 64, 5)
    feat[10:20] = 0.0                      # p = 0 for these rows
    lo[1] = hi[1] = 0.0                    # channel 1: (p - 0) / 0
    feat[30, 5] = np.nan
    feat[31, 7] = np.inf
    for s in (None, scale):
        got = host(ops.feature_colours(dev(feat), dev(mat), dev(lo), dev(hi), None if s is None else dev(s)))
        ref, bound = C.feature_colours(feat, mat, lo, hi, s)
        assert np.isnan(ref[10:20, 1]).all() and np.isnan(ref[30]).all()
        assert set(np.unique(ref[40:, 1] / (1.0 if s is None else s[40:].astype(np.float64)))) == {0.0, 1.0}
        C.assert_within(got, ref, bound, f"degenerate range, scale={s is not None}")


def test_feature_colours_do_not_depend_on_the_launch(hip_lib):
    """Bit for bit: rows [0:k] of a call on N rows == a call on the first k rows; a job alone == the job as a member of a 6-job
    launch; an unaligned view (row 1 of E = 3 / E = 65: no 16-byte alignment) == the aligned copy; E = 64 read through the scalar
    path (a view at a 4-byte offset) == the 16-byte path; two calls agree."""
    from emernerf_amd import ops
    for E in (64, 768, 3):
        feat, mat, lo, hi, scale = (dev(a) for a in _random_case(4097, E, 7 + E))
        full = ops.feature_colours(feat, mat, lo, hi, scale)
        assert torch.equal(full, ops.feature_colours(feat, mat, lo, hi, scale))
        for k in (1, 64, 1000):
            assert torch.equal(full[:k], ops.feature_colours(feat[:k], mat, lo, hi, scale[:k])), (E, k)
        others = [(feat.flip(0) * (j + 1), mat, lo, hi, None if j % 2 else scale) for j in range(5)]
        multi = ops.feature_colours_multi(others[:2] + [(feat, mat, lo, hi, scale)] + others[2:])
        assert len(multi) == 6 and torch.equal(multi[2], full), E
        for j, o in enumerate(others):
            assert torch.equal(multi[j if j < 2 else j + 1], ops.feature_colours(*o)), (E, j)
    for E in (3, 65):
        feat, mat, lo, hi, _ = (dev(a) for a in _random_case(130, E, 9 + E))
        view = feat[1:]
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        assert torch.equal(ops.feature_colours(view, mat, lo, hi), ops.feature_colours(view.clone(), mat, lo, hi)), E
        assert torch.equal(ops.feature_colours(view, mat, lo, hi), ops.feature_colours(feat, mat, lo, hi)[1:]), E
    feat, mat, lo, hi, _ = (dev(a) for a in _random_case(300, 64, 21))
    shifted = torch.empty(300 * 64 + 1, device=DEV)[1:].view(300, 64)
    shifted.copy_(feat)
    assert shifted.data_ptr() % 16 == 4 and feat.data_ptr() % 16 == 0
    assert torch.equal(ops.feature_colours(shifted, mat, lo, hi), ops.feature_colours(feat, mat, lo, hi))


def test_blend_over_vs_float64(hip_lib):
    from emernerf_amd import ops
    rng = np.random.default_rng(3)
    for N in (1, 85, 4097):
        a, b = rng.random((N, 3)).astype(np.float32) * 1.4 - 0.2, rng.random((N, 3)).astype(np.float32) * 1.4 - 0.2
        o = rng.random(N).astype(np.float32)
        o[: N // 8] = 0.0
        o[N // 8: N // 4] = 1.0
        ref, bound = C.blend_over(a, o, b)
        got = ops.blend_over(dev(a), dev(o).reshape(N, 1), dev(b))
        C.assert_within(host(got), ref, bound, f"blend N={N}")
    a[0, 0] = np.nan
    got = host(ops.blend_over(dev(a), dev(o), dev(b)))
    assert np.isnan(got[0, 0]) and not np.isnan(got[0, 1:]).any()
    two = ops.blend_over_multi([(dev(a), dev(o), dev(b)), (dev(b), dev(o), dev(a))])
    assert np.array_equal(host(two[0]), got, equal_nan=True)
    assert np.array_equal(host(two[1]), host(ops.blend_over(dev(b), dev(o), dev(a))), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------- the loop
def _replay_case(pe):
    """The recorded feature model as a render_func: image i's recorded raw results, uploaded and CAPTURED."""
    z, tag, images = load_feature_case(pe)
    images = [{k: v.to(DEV) for k, v in d.items()} for d in images]
    model = types.SimpleNamespace(feats_reduction_mat=dev(z[tag + "reg/mat"]), feat_color_min=dev(z[tag + "reg/lo"]),
                                  feat_color_max=dev(z[tag + "reg/hi"]))
    captured = []

    def render_func(data):
        i = len(captured) % len(images)
        res = {k[len(f"{tag}raw/{i}/"):]: dev(z[k]) for k in z.files if k.startswith(f"{tag}raw/{i}/")}
        captured.append(res)
        return res
    pca = None
    if pe:
        pca = {n: tuple(dev(z[f"{tag}pca/{n}/{k}"]) for k in ("mat", "lo", "hi")) for n in ("pe_free", "pe")}
    return z, tag, images, model, render_func, captured, pca


@pytest.mark.parametrize("pe", [1, 0])
def test_loop_feature_lists_are_the_ops_on_the_raw_results(hip_lib, pe):
    """render(visualize=True) on the recorded feature model: every new list equals, bit for bit, the ops applied to the captured
    raw results in the reference's order; the non-empty lists are the recording's; the launch budget holds (one projection
    launch, one blend launch, one flow launch per image)."""
    from torch.profiler import ProfilerActivity, profile
    from emernerf_amd import video_utils
    z, tag, images, model, render_func, captured, pca = _replay_case(pe)
    out = video_utils.render(G.GoldenSplit(images), render_func, model=model, visualize=True, feature_pca=pca)   # (warm-up of the launch count)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = video_utils.render(G.GoldenSplit(images), render_func, model=model, visualize=True, feature_pca=pca)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.device_time_total > 0]
    n = len(images)
    assert sum("feature_colours_kernel" in s for s in names) == n, names
    assert sum("blend_over_kernel" in s for s in names) == n, names
    assert sum("flow_colours_kernel" in s for s in names) == n, names
    want = {k[len(tag) + 4:] for k in z.files if k.startswith(tag + "len/") and int(z[k]) > 0}
    got = {k for k, v in out.items() if isinstance(v, list) and len(v) > 0}
    assert got == want, (sorted(got - want), sorted(want - got))
    assert ("feature_pca" in out) == bool(pe)
    from emernerf_amd import ops
    for i, d in enumerate(images):
        exp = _ops_lists(z, tag, i, d["features"].cpu().numpy())
        for k in ("forward_flow", "backward_flow"):
            exp[k + "s"] = ops.flow_colours(captured[i][k], 1.0, "bright")
        assert len(exp) == (10 if pe else 8)
        for name, t in exp.items():
            a = out[name][i]
            assert len(out[name]) == n and a.dtype == np.float32 and a.shape == (5, 7, 3), (name, a.shape)
            assert np.array_equal(a, host(t).reshape(a.shape), equal_nan=True), f"{tag}{name}[{i}]"


def test_loop_computes_and_returns_the_pca_when_none_is_given(hip_lib):
    """feature_pca=None: the matrices come from the first image (get_robust_pca, sky zeroed, m = 2.5), are returned, and a second
    call given them reproduces the first bit for bit."""
    from emernerf_amd import video_utils
    z, tag, images, model, render_func, captured, _ = _replay_case(1)
    out = video_utils.render(G.GoldenSplit(images), render_func, model=model, visualize=True)
    pca = out["feature_pca"]
    raw0 = captured[0]
    non_sky = raw0["dino_pe_free"] * (~images[0]["sky_masks"].bool().unsqueeze(-1)).float()
    want = {"pe_free": video_utils.get_robust_pca(non_sky.reshape(-1, 64), m=2.5), "pe": video_utils.get_robust_pca(raw0["dino_pe"].reshape(-1, 64), m=2.5)}
    for n in ("pe_free", "pe"):
        assert all(torch.equal(a, b) for a, b in zip(pca[n], want[n])), n
        assert pca[n][0].shape == (64, 3) and pca[n][0].is_cuda and bool((pca[n][2] > pca[n][1]).all())
    again = video_utils.render(G.GoldenSplit(images), render_func, model=model, visualize=True, feature_pca=pca)
    for k in ("dino_feats_pe_free", "dino_pe", "static_dino_feats", "dynamic_dino_on_static_rgbs"):
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(out[k], again[k])), k


def _flow_model():
    from emernerf_amd.prop_net import PropNetEstimator
    from emernerf_amd.radiance_field import build_density_field, build_radiance_field_from_cfg
    gold = np.load(os.path.join(GOLDEN, "render_pixels_flow.npz"))
    cfg = G.model_cfg("flow")
    torch.manual_seed(0)
    model = build_radiance_field_from_cfg(cfg, verbose=False)
    props = [build_density_field(aabb=G.AABB, unbounded=True, **k) for k in G.PROP_KW]
    seed = int(gold["table_seed"])
    for prefix, m in [("model/", model)] + [(f"prop{i}/", p) for i, p in enumerate(props)]:
        sd = {k: (G.table_values(prefix + k, v.numel(), seed) if k.endswith("tcnn_encoding.params")
                  else torch.from_numpy(gold["state/" + prefix + k])) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        m.to(DEV)
    model.time_diff = 1 / cfg.num_train_timesteps
    est = PropNetEstimator(None, None).to(DEV)
    n_img = len({k.split("/")[0] for k in gold if k.startswith("image")})
    images = [{k[len(f"image{i}/"):]: torch.from_numpy(v).to(DEV) for k, v in gold.items() if k.startswith(f"image{i}/")} for i in range(n_img)]
    return gold, model, props, est, images


def test_loop_flow_model_colours_and_unchanged_default(hip_lib):
    """The flow model of render_pixels_flow.npz: with visualize=True the flow lists are ops.flow_colours of the captured raw
    flows, bit for bit, and every other list is unchanged; visualize=False equals a call without the keyword (same keys, same
    arrays, raw flows -- the reference's recording made with an identity visualiser --, no feature_pca key)."""
    from emernerf_amd import ops, video_utils
    from emernerf_amd.render_utils import render_rays
    gold, model, props, est, images = _flow_model()
    rcfg = G.render_cfg([24, 16], 16, chunk=25)
    model.eval()
    for p in props:
        p.eval()
    est.eval()
    captured = []

    def render_func(data):
        res = render_rays(radiance_field=model, proposal_estimator=est, proposal_networks=props, data_dict=data, cfg=rcfg, return_decomposition=True)
        captured.append({k: res[k].clone() for k in ("forward_flow", "backward_flow")})
        return res
    vis = video_utils.render(G.GoldenSplit(images), render_func, model=model, visualize=True)
    assert "feature_pca" not in vis and "dino_feats" not in vis
    for k in ("forward_flow", "backward_flow"):
        assert len(vis[k + "s"]) == len(images)
        for i in range(len(images)):
            assert np.array_equal(vis[k + "s"][i], host(ops.flow_colours(captured[i][k], 1.0, "bright")))
            assert vis[k + "s"][i].min() >= 0.0 and vis[k + "s"][i].max() <= 1.0
    kw = dict(proposal_networks=props, compute_metrics=True, return_decomposition=True)
    plain = video_utils.render_pixels(rcfg, model, est, G.GoldenSplit(images), **kw)
    off = video_utils.render_pixels(rcfg, model, est, G.GoldenSplit(images), visualize=False, feature_pca=None, **kw)
    on = video_utils.render_pixels(rcfg, model, est, G.GoldenSplit(images), visualize=True, **kw)
    assert list(plain) == list(off) and "feature_pca" not in off
    for k, v in plain.items():
        if k == "render_rays_per_s":
            continue
        if isinstance(v, list):
            assert len(v) == len(off[k]) and all(np.array_equal(a, b) for a, b in zip(v, off[k])), k
            if k not in ("forward_flows", "backward_flows"):
                assert all(np.array_equal(a, b) for a, b in zip(v, on[k])), k
        else:
            assert v == off[k] and v == on[k], k
    assert set(on) == set(plain)
    for i in range(len(images)):       # the default keeps the RAW flow
        assert np.array_equal(plain["forward_flows"][i], host(captured[i]["forward_flow"]).squeeze())
        assert not np.array_equal(plain["forward_flows"][i], on["forward_flows"][i])
