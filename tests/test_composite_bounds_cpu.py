"""The compositing tests' own power, without a GPU: the numpy model of the kernels (tests/_composite_model.py) against the
exact probes (tests/_composite_probe.py) and the per-entry bounds (tests/_bounds.py render_bounds, dsigma_bound,
epilogue_bounds, c_accumulate, blend_c).

* every probe meets its preconditions (the builders assert them) and the fp32 model equals the fp64 restatement on it,
  entry by entry, for every family: walls, accumulate, both blends, the epilogue;
* the model is inside every bound on the realistic inputs the GPU test uses, and no ray of the committed seeds has a
  cumsum of w within its bound of 0.5 (the GPU test holds the median exactly, without a skip);
* every mutant of ``MUTANTS`` differs on at least one probe, and on the probe aimed at it (named below);
* the closed-form fp64 reverse mode is torch's fp64 autograd of the forward expressions.
"""
import numpy as np
import pytest
import torch

from tests import _bounds as B
from tests import _composite_model as M
from tests import _composite_probe as P


def _rots(S, R):
    n = len(P.wall_configs(S))
    return range(0, n, R) if R < n else range(1)


@pytest.mark.parametrize("R", P.WALL_R)
@pytest.mark.parametrize("S", P.WALL_S)
def test_wall_probes_model_equals_fp64(S, R):
    seen = set()
    for rot in _rots(S, R):
        p = P.wall_probe(R, S, rot)
        seen.update(p["walls"])
        what = f"wall S={S} R={R} rot={rot}"
        P.check_wall_render(p, M.model_render(p), what)
        P.check_wall_composite(p, M.model_composite(p), what + " fused")
        # the model in float64 is the restatement too (to rounding): the structure computes the same function
        np.testing.assert_allclose(M.model_render(p, dt=P.F64)["d_sigma"], P.ref_render_all(p)[1]["d_sigma"], rtol=1e-12, atol=1e-12)
    assert seen == set(P.wall_configs(S)), "a wall position is never run"


@pytest.mark.parametrize("R", P.ACC_R)
@pytest.mark.parametrize("S", P.ACC_S)
def test_accumulate_probes_model_equals_fp64(S, R):
    for C in P.ACC_C:
        p = P.accumulate_probe(R, S, C)
        P.check_accumulate(p, *M.model_accumulate(p["w"], p["v"], p["go"]), f"accumulate S={S} R={R} C={C}")


@pytest.mark.parametrize("S", P.BLEND_S)
@pytest.mark.parametrize("with_shadow", [True, False])
def test_blend_probes_model_equals_fp64(S, with_shadow):
    for R in (1, 5):
        p = P.blend_probe(R, S, with_shadow)
        P.check_blend(p, M.model_blend(p), f"blend S={S} R={R} shadow={with_shadow}")


@pytest.mark.parametrize("S", P.WIDE_S)
def test_wide_blend_probes_model_equals_fp64(S):
    straddle = False
    for R in P.WIDE_R:
        for C in P.WIDE_C:
            p = P.blend_wide_probe(R, S, C)
            P.check_blend(p, M.model_blend_wide(p), f"wide S={S} R={R} C={C}", wide=True)
        straddle |= R > 1 and S % 4 != 0 and (R * S) % 4 != 0
    if S in (1, 3, 5, 7, 9, 13, 129):
        assert straddle, "no case whose quads straddle two rays with a ragged end"


def test_wide_cap_case_reaches_the_workgroup_cap():
    R, S, C = P.WIDE_CAP
    assert -(-R * S // 32) > 16384 and S % 4 != 0 and (R * S) % 4 != 0 and R * S * C * 4 < 8 << 20
    P.blend_wide_probe(R, S, C)


def _model_epilogue(p, mut=""):
    o, dep, med, rgb = M.model_epilogue_fwd(p["stats"], p["acc"], p["sky"])
    g0, g1, dsky = M.model_epilogue_bwd(p["stats"], p["sky"], p["d_opa"], p["d_dep"], p["d_out"], mut)
    z = np.zeros_like(g0)
    return dict(opacity=o, depth=dep, median=med, rgb=rgb, d_stats=np.stack([g0, g1, z, z], 1), d_acc=p["d_out"], d_sky=dsky)


def test_epilogue_probe_model():
    p = P.epilogue_probe()
    assert set(p["stats"][:, 0].tolist()) == set(float(x) for x in P.SPECIAL_WSUM)
    P.check_epilogue_probe(p, _model_epilogue(p), "epilogue")


# ------------------------------------------------------------------------------------------------------------ mutants
def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _wall_cases():
    for S in (2, 63, 65, 129, 200):
        for R in (5, 13):
            for rot in _rots(S, R):
                yield S, R, rot


# mutant -> the probe that must catch it (family and S, matched as whole words: "wall S=2" is not "wall S=200")
AIMED = {
    "carry2": "wall S=129", "carry_prev": "wall S=129", "incl": "wall S=2", "suffix": "wall S=65", "tail": "wall S=63",
    "latch": "wall S=65", "lane63": "wall S=63", "dalpha": "wall S=2", "strict": "epilogue", "acc_tail": "accumulate S=65",
    "wide_tail": "wide S=5", "quad_ray": "wide S=5",
}


@pytest.mark.parametrize("name", list(M.MUTANTS))
def test_every_mutant_differs_on_a_named_probe(name):
    caught = []
    if name in ("acc_tail",):
        for S in P.ACC_S:
            for C in (None, 1, 3, 8):
                p = P.accumulate_probe(5, S, C)
                if _fails(lambda: P.check_accumulate(p, *M.model_accumulate(p["w"], p["v"], p["go"], name), "m")):
                    caught.append(f"accumulate S={S} C={C}")
    elif name in ("wide_tail", "quad_ray"):
        for S in P.WIDE_S:
            for C in (1, 65):
                p = P.blend_wide_probe(3, S, C)
                if _fails(lambda: P.check_blend(p, M.model_blend_wide(p, name), "m", wide=True)):
                    caught.append(f"wide S={S} C={C}")
    else:
        if name == "strict":
            p = P.epilogue_probe()
            if _fails(lambda: P.check_epilogue_probe(p, _model_epilogue(p, name), "m")):
                caught.append("epilogue")
        for S, R, rot in _wall_cases():
            p = P.wall_probe(R, S, rot)
            bad = _fails(lambda: P.check_wall_composite(p, M.model_composite(p, name), "m"))
            if name != "strict":
                bad |= _fails(lambda: P.check_wall_render(p, M.model_render(p, name), "m"))
            if bad:
                caught.append(f"wall S={S} R={R} rot={rot}")
    print(f"\n[mutant] {name} ({M.MUTANTS[name]}): differs on {len(caught)} probes: {', '.join(caught[:12])}")
    assert caught, f"mutant {name} passes every probe"
    aimed = AIMED[name]
    assert any(c == aimed or c.startswith(aimed + " ") for c in caught), f"mutant {name} is not caught by {aimed}: {caught}"


# --------------------------------------------------------------------------------------------------- realistic inputs
def _report(rep, what):
    print(f"\n[worst err / bound] {what}: " + ", ".join(f"{k.split(' ', 1)[1] if ' ' in k else k} {v:.3g}" for k, v in rep.items()))


@pytest.mark.parametrize("R,S", P.REAL_SHAPES)
def test_model_is_inside_the_bounds_on_realistic_rays(R, S):
    p = P.realistic(R, S)
    assert (p["sg"][0] == 0).all() and (R < 2 or (p["sg"][1] == 50).all())
    rep = {}
    rf, bd = P.check_real_render(p, M.model_render(p), f"model R={R} S={S}", rep)
    # the zero-ambiguous-median condition for the committed seed (check_real_render asserts it; stated here for the record)
    assert not B.median_ambiguous(rf, bd).any()
    P.check_real_composite(p, M.model_composite(p), f"model fused R={R} S={S}", rep, wsum=M.model_render(p)["stats"][:, 0])
    _report(rep, f"model R={R} S={S}")
    # the bound separates: every scan mutant that changes a value on these inputs leaves it
    for name in ("carry2", "carry_prev", "incl", "suffix", "dalpha"):
        changed = not np.array_equal(M.model_render(p, name)["d_sigma"], M.model_render(p)["d_sigma"])
        if changed:
            assert _fails(lambda: P.check_real_render(p, M.model_render(p, name), "m")), f"mutant {name} stays inside the bound"
    # ... in the fused kernel too, on every ray -- those whose fp32 sum w takes the other clamp branch than fp64 included
    base = M.model_composite(p)["d_sigma"]
    # (S = 1: g0 and g1 mid cancel in gw, the bound is on their abs-sum and a 0.1 % slip stays inside it; the probes hold S = 1)
    for name in ("carry_prev", "incl", "suffix") if S > 1 else ():
        mut = M.model_composite(p, name)
        big = np.abs(mut["d_sigma"] - base).max(1) > 1e-3 * np.abs(base).max(1)      # (a slip of rounding size cannot show)
        for r in np.flatnonzero(big):
            one = dict(mut, d_sigma=np.where(np.arange(R)[:, None] == r, mut["d_sigma"], base))   # the slip on ray r alone
            only = dict(M.model_composite(p), d_sigma=one["d_sigma"])
            assert _fails(lambda: P.check_real_composite(p, only, "m", wsum=M.model_render(p)["stats"][:, 0])), \
                f"fused mutant {name} stays inside the bound on ray {r}"


@pytest.mark.parametrize("C", [None, 1, 3, 6, 9, 64, 100])
def test_model_accumulate_and_blends_inside_the_bounds(C):
    rng = np.random.default_rng(7)
    R, S = 5, 130
    p = dict(w=rng.random((R, S)).astype(P.F32), v=None if C is None else rng.standard_normal((R, S, C)).astype(P.F32),
             go=rng.standard_normal((R, C or 1)).astype(P.F32))
    rep = {}
    P.check_real_accumulate(p, *M.model_accumulate(p["w"], p["v"], p["go"]), f"model accumulate C={C}", rep)
    if C in (3, 64, 100):
        q = P.realistic_blend(R, S, None if C == 3 else C)
        P.check_real_blend(q, M.model_blend(q) if C == 3 else M.model_blend_wide(q), f"model blend C={C}", wide=C != 3, report=rep)
    _report(rep, f"model C={C}")


def test_closed_form_reverse_mode_is_fp64_autograd():
    p = P.realistic(4, 70)
    def t(k):
        return torch.from_numpy(np.asarray(p[k], np.float64))
    ts, te, rgb, sky = t("ts"), t("te"), t("rgb"), t("sky")
    sg = t("sg").requires_grad_(True)
    x = sg * (te - ts)
    excl = torch.cumsum(x, 1) - x
    T, al = torch.exp(-excl), 1 - torch.exp(-x)
    w = T * al
    mid = (ts + te) / 2
    cd = torch.cat([1 - T, torch.ones(4, 1, dtype=torch.float64)], 1)
    st = torch.stack([w.sum(1), (w * mid).sum(1)], 1)
    ((w * t("dW")).sum() + (T * t("dT")).sum() + (al * t("dA")).sum() + (cd * t("dC")).sum() + (st * t("dS")[:, :2]).sum()).backward()
    rf, g = P.ref_render_all(p)
    np.testing.assert_allclose(g["d_sigma"], sg.grad.numpy(), rtol=1e-9, atol=1e-12)
    sg.grad = None
    c, k = rgb.clone().requires_grad_(True), sky.clone().requires_grad_(True)
    x = sg * (te - ts)
    T = torch.exp(-(torch.cumsum(x, 1) - x))
    w = T * (1 - torch.exp(-x))
    o = w.sum(1, keepdim=True).clamp(float(P.EPS), 1.0)
    dep = (w * mid).sum(1, keepdim=True) / o
    out = (w[..., None] * c).sum(1) + k * (1 - o)
    ((o * t("d_opa")).sum() + (dep * t("d_dep")).sum() + (out * t("d_out")).sum() + (w * t("dW")).sum() + (T * t("dT")).sum()).backward()
    rf, ep, g = P.ref_composite_all(p)
    ok = ep["passes"]       # (the saturated ray's fp64 sum may round above 1: torch cuts it as the restatement does)
    np.testing.assert_allclose(g["d_sigma"][ok], sg.grad.numpy()[ok], rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(ep["d_rgb"], c.grad.numpy(), rtol=1e-9, atol=1e-14)   # (torch forms excl as cumsum - x: it cancels)
    np.testing.assert_allclose(ep["d_sky"], k.grad.numpy(), rtol=1e-9, atol=1e-14)    # (torch sums w: 1 - o cancels)
    np.testing.assert_allclose(out.detach().numpy(), ep["rgb"], rtol=1e-12)
