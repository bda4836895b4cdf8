"""CPU checks of the evaluation colours: the product's colour wheel against the reference's, the reference's OWN recorded
colours against the float64 restatements and bounds of tests/_colour_ref.py (the bounds the kernels are held to in
tests/test_colours_gpu.py are ones the reference itself meets on these inputs), and ``video_utils.get_robust_pca``."""
import os

import numpy as np
import torch

from tests import _colour_ref as C
from tests.golden import record_colours as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_feature_case(pe):
    """(fixture, prefix, per-image inputs regenerated from the seed) of the PE-on / PE-off recording."""
    z = np.load(os.path.join(GOLDEN, "feature_colours.npz"))
    return z, f"pe{pe}/", RC.feature_images(**RC.FEATURE_COLOURS)


def expected_feature_lists(z, tag, i, features, colour_fn, blend_fn, lists=None):
    """{list: value} of image ``i`` from the recorded raw results in the reference's order (video_utils.py:233-418), with
    ``colour_fn(feat, (mat, lo, hi), scale)`` and ``blend_fn(a, o, b)`` supplied by the caller (restatement or ops).  The blends
    read two of the colour lists: ``lists(name)`` supplies them (default: the values computed here)."""
    raw = lambda k: z[f"{tag}raw/{i}/{k}"]  # noqa: E731
    has = lambda k: f"{tag}raw/{i}/{k}" in z.files  # noqa: E731
    reg = tuple(z[tag + "reg/" + k] for k in ("mat", "lo", "hi"))
    out = {"dino_feats": colour_fn(raw("dino_feat"), reg, None), "gt_dino_feats": colour_fn(features, reg, None)}
    if has("dino_pe_free"):
        free = tuple(z[tag + "pca/pe_free/" + k] for k in ("mat", "lo", "hi"))
        pe = tuple(z[tag + "pca/pe/" + k] for k in ("mat", "lo", "hi"))
        out["dino_feats_pe_free"] = colour_fn(raw("dino_pe_free"), free, raw("opacity"))
        out["dino_pe"] = colour_fn(raw("dino_pe"), pe, None)
        out["static_dino_feats"] = colour_fn(raw("static_dino"), free, None)
        out["dynamic_dino_feats"] = colour_fn(raw("dynamic_dino"), free, raw("dynamic_opacity"))
    else:
        out["static_dino_feats"] = colour_fn(raw("static_dino"), reg, None)
        out["dynamic_dino_feats"] = colour_fn(raw("dynamic_dino"), reg, None)
    lists = lists or out.__getitem__
    out["dynamic_rgb_on_static_dinos"] = blend_fn(raw("dynamic_rgb"), raw("dynamic_opacity"), lists("static_dino_feats"))
    out["dynamic_dino_on_static_rgbs"] = blend_fn(lists("dynamic_dino_feats"), raw("dynamic_opacity"), raw("static_rgb"))
    return out


def test_wheel_equals_the_reference_wheel():
    from emernerf_amd import ops
    z = np.load(os.path.join(GOLDEN, "flow_colours.npz"))
    w = ops.colour_wheel()
    assert w.dtype == np.float32 and w.shape == (56, 3) and int(z["N_COLS"]) == C.N_COLS
    np.testing.assert_array_equal(w, z["WHEEL"])
    np.testing.assert_array_equal(w[0], w[-1])


def test_reference_flow_colours_meet_the_bound():
    """Every row of the recording (zero flow, on and next to wheel nodes, radius 1 +- a hair, radius 5, negative y, random),
    both backgrounds, within 1e-5 of the float64 restatement."""
    z = np.load(os.path.join(GOLDEN, "flow_colours.npz"))
    np.testing.assert_array_equal(z["flow"], RC.flow_batch())
    assert len(z["flow"]) >= 200
    for bg in ("bright", "dark"):
        ref = C.flow_colours(z["flow"], z["WHEEL"], 1.0, bg)
        assert ref.min() >= -1e-12 and ref.max() <= 1.0 + 1e-12
        C.assert_within(z["rgb/" + bg], ref, C.FLOW_BOUND, "reference flow colours, " + bg)
    bright = C.flow_colours(z["flow"][:1], z["WHEEL"], 1.0, "bright")
    dark = C.flow_colours(z["flow"][:1], z["WHEEL"], 1.0, "dark")
    assert (bright == 1.0).all() and (dark == 0.0).all()      # zero flow: white on "bright", black on "dark"


def test_reference_feature_colours_meet_the_bounds():
    """Every colour list the reference's loop returned, PE on and PE off, the two blends and the loop's flow images included,
    within the bounds of the float64 restatement of the same recorded inputs."""
    checked = 0
    for pe in (1, 0):
        z, tag, images = load_feature_case(pe)
        want_lists = {"dino_feats", "gt_dino_feats", "static_dino_feats", "dynamic_dino_feats", "dynamic_rgb_on_static_dinos",
                      "dynamic_dino_on_static_rgbs"} | ({"dino_feats_pe_free", "dino_pe"} if pe else set())
        for i, d in enumerate(images):
            rec = lambda k: z[f"{tag}res/{k}/{i}"]  # noqa: E731

            def colour(feat, pca, scale):
                return C.feature_colours(feat, *pca, scale)

            # the blends' inputs are the reference's own recorded lists (fp32 values): no bound is carried in
            exp = expected_feature_lists(z, tag, i, d["features"].numpy(), colour, C.blend_over, lists=rec)
            assert set(exp) == want_lists
            for name, (ref, bound) in exp.items():
                C.assert_within(rec(name), ref.reshape(rec(name).shape), bound.reshape(rec(name).shape), f"{tag}{name}[{i}]")
                checked += 1
            for k in ("forward_flow", "backward_flow"):
                ref = C.flow_colours(z[f"{tag}raw/{i}/{k}"], C._f64(np.load(os.path.join(GOLDEN, "flow_colours.npz"))["WHEEL"]), 1.0, "bright")
                C.assert_within(rec(k + "s"), ref.reshape(rec(k + "s").shape), C.FLOW_BOUND, f"{tag}{k}s[{i}]")
        got_lists = {k[len(tag) + 4:] for k in z.files if k.startswith(tag + "len/") and int(z[k]) > 0}
        assert want_lists <= got_lists
        assert ("dino_pe" in got_lists) == bool(pe)
    assert checked == 2 * (8 + 6)


def _pca_features(n, e, seed, dtype=torch.float32):
    """Seeded features with well-separated leading singular values (after centring) and a mean far from zero."""
    g = torch.Generator().manual_seed(seed)
    basis, _ = torch.linalg.qr(torch.randn(e, e, generator=g, dtype=torch.float64))
    sv = torch.cat([torch.tensor([9.0, 5.0, 2.5], dtype=torch.float64), 0.3 * torch.rand(e - 3, generator=g, dtype=torch.float64)])
    x = torch.randn(n, e, generator=g, dtype=torch.float64) * sv @ basis.T + 3.0 * torch.randn(e, generator=g, dtype=torch.float64)
    return x.to(dtype)


def test_get_robust_pca_is_the_deterministic_restatement():
    from emernerf_amd.video_utils import get_robust_pca
    for n, e, seed, m in ((500, 16, 1, 2.5), (300, 64, 2, 2.0)):
        x = _pca_features(n, e, seed)
        mat, lo, hi = get_robust_pca(x, m=m)
        assert mat.shape == (e, 3) and mat.dtype == x.dtype and lo.shape == hi.shape == (3,) and lo.dtype == x.dtype
        x64 = x.numpy().astype(np.float64)
        _, s, vt = np.linalg.svd(x64 - x64.mean(0), full_matrices=False)
        assert s[2] / s[3] > 2 and s[0] / s[1] > 1.3 and s[1] / s[2] > 1.3
        v = mat.numpy().astype(np.float64)
        assert np.abs(v @ v.T - vt[:3].T @ vt[:3]).max() <= 1e-6
        for c in range(3):      # the columns in order of decreasing variance, each with its largest-magnitude entry positive
            assert abs(abs(v[:, c] @ vt[c]) - 1.0) <= 1e-6
            assert v[np.abs(v[:, c]).argmax(), c] > 0
        colors = (x @ mat).numpy()                 # the UNCENTRED product
        want_lo, want_hi = C.robust_range(colors, m)
        np.testing.assert_allclose(lo.numpy(), want_lo, rtol=1e-6)
        np.testing.assert_allclose(hi.numpy(), want_hi, rtol=1e-6)
        assert (lo.numpy() > colors.min(0)).any() or (hi.numpy() < colors.max(0)).any()   # the rule trims outliers
        again = get_robust_pca(x.clone(), m=m)
        assert all(torch.equal(a, b) for a, b in zip((mat, lo, hi), again))
