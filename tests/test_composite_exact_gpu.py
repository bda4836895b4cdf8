"""The compositing kernels (csrc/composite.hip, the ray epilogue of csrc/rayloss.hip) held to exact probes and per-entry
fp64 bounds.  tests/_composite_probe.py has the probes, the fp64 restatement and the argument; tests/_bounds.py the bounds;
tests/test_composite_bounds_cpu.py shows what the probes catch (the numpy model of tests/_composite_model.py, twelve mutants).

* wall probes (sigma dt is 0 or 128: T, alpha and w are 0 or 1) for render_weights and composite_rgb, dyadic probes for
  accumulate, both blends and the epilogue: every output and gradient equals the fp64 reference rounded to fp32, entry by
  entry, at S from 1 to 4096 (chunk_base exactly full), partial workgroups, every residue of the wide loops;
* realistic rays: every entry of every output and gradient inside its first-order bound, the median exact, composite_rgb
  against the fp64 restatement directly; the worst err / bound is printed per output (DESIGN.md 4.4 records them);
* what the kernels' shared stages rely on: a null optional output or upstream gradient changes no other result;
* the argument contract of the entry points.
"""
import numpy as np
import pytest
import torch

from tests import _composite_probe as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _d(a, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)
    return t.requires_grad_(True) if grad else t


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def _rots(S, R):
    n = len(P.wall_configs(S))
    return range(0, n, R) if R < n else range(1)


def run_render(p):
    from emernerf_amd import ops
    sg = _d(p["sg"], True)
    w, T, a, cdfs, stats, tm, td = ops.render_weights(_d(p["ts"]), _d(p["te"]), sg, want_t=True)
    ((w * _d(p["dW"])).sum() + (T * _d(p["dT"])).sum() + (a * _d(p["dA"])).sum() + (cdfs * _d(p["dC"])).sum()
     + (stats * _d(p["dS"])).sum()).backward()     # (columns 2, 3 of d stats hold 7: the kernel must not read them)
    return dict(weights=_n(w), trans=_n(T), alphas=_n(a), cdfs=_n(cdfs), stats=_n(stats), t_mid=_n(tm), t_dist=_n(td), d_sigma=_n(sg.grad))


def run_composite(p, with_rgb=True, with_sky=True):
    from emernerf_amd import ops
    sg = _d(p["sg"], True)
    c = _d(p["rgb"], True) if with_rgb else None
    sk = _d(p["sky"], True) if (with_rgb and with_sky) else None
    w, T, tm, td, opa, dep, med, out = ops.composite_rgb(_d(p["ts"]), _d(p["te"]), sg, c, sk)
    loss = (opa * _d(p["d_opa"])).sum() + (dep * _d(p["d_dep"])).sum() + (w * _d(p["dW"])).sum() + (T * _d(p["dT"])).sum()
    if out is not None:
        loss = loss + (out * _d(p["d_out"])).sum()
    loss.backward()
    return dict(weights=_n(w), trans=_n(T), t_mid=_n(tm), t_dist=_n(td), opacity=_n(opa)[:, 0], depth=_n(dep)[:, 0], median=_n(med)[:, 0],
                rgb_out=_n(out), d_sigma=_n(sg.grad), d_rgb=None if c is None else _n(c.grad), d_sky=None if sk is None else _n(sk.grad))


def _strip(p, with_rgb, with_sky):
    q = dict(p)
    if not with_rgb:
        q.update(rgb=None, sky=None, d_out=None)
    elif not with_sky:
        q.update(sky=None)
    return q


# ------------------------------------------------------------------------------------------------------- exact probes
@pytest.mark.parametrize("R", P.WALL_R)
@pytest.mark.parametrize("S", P.WALL_S)
def test_wall_probes_exact(hip_lib, S, R):
    """render_weights and composite_rgb on the wall probes: every wall position (none, 0, 1, 62 .. 65, 127, 128, S - 1, two
    walls in two chunks) on some ray; R = 5, 13 leave a partial workgroup; S = 4096 fills chunk_base."""
    for rot in _rots(S, R):
        p = P.wall_probe(R, S, rot)
        what = f"wall S={S} R={R} rot={rot}"
        P.check_wall_render(p, run_render(p), what)
        P.check_wall_composite(p, run_composite(p), what + " fused")
    P.check_wall_composite(_strip(p, True, False), run_composite(p, True, False), what + " fused, no sky")
    P.check_wall_composite(_strip(p, False, False), run_composite(p, False, False), what + " fused, geometry only")


def run_accumulate(p):
    from emernerf_amd import ops
    w, v = _d(p["w"], True), _d(p["v"], True)
    out = ops.accumulate_along_rays(w, v)
    out.backward(_d(p["go"]))
    return _n(out), _n(w.grad), None if v is None else _n(v.grad)


@pytest.mark.parametrize("R", P.ACC_R)
@pytest.mark.parametrize("S", P.ACC_S)
def test_accumulate_probes_exact(hip_lib, S, R):
    """Every small-kernel instantiation (C = 1 .. 8 and values None), the wide kernel at C = 9, 64, 65, 100, 129."""
    for C in P.ACC_C:
        p = P.accumulate_probe(R, S, C)
        P.check_accumulate(p, *run_accumulate(p), f"accumulate S={S} R={R} C={C}")


def run_blend(p):
    from emernerf_amd import ops
    names = ("w", "sig", "ss", "sd", "rs", "rd", "sh")
    t = {k: _d(p[k], True) for k in names}
    acc, acs = ops.blend_accumulate(*(t[k] for k in names))
    loss = (acc * _d(p["g_rgb"])).sum()
    if acs is not None:
        loss = loss + (acs * _d(p["g_sh"])).sum()
    loss.backward()
    got = {"d_" + k: _n(t[k].grad) for k in names if t[k] is not None}
    got.update(acc=_n(acc), acs=None if acs is None else _n(acs)[:, 0])
    return got


@pytest.mark.parametrize("S", P.BLEND_S)
@pytest.mark.parametrize("with_shadow", [True, False])
def test_blend_probes_exact(hip_lib, S, with_shadow):
    for R in (1, 5):
        p = P.blend_probe(R, S, with_shadow)
        P.check_blend(p, run_blend(p), f"blend S={S} R={R} shadow={with_shadow}")


def run_blend_wide(p):
    from emernerf_amd import ops
    names = ("w", "sig", "ss", "sd", "fs", "fd")
    t = {k: _d(p[k], True) for k in names}
    acc = ops.blend_accumulate_wide(*(t[k] for k in names))
    acc.backward(_d(p["g_acc"]))
    got = {"d_" + k: _n(t[k].grad) for k in names}
    got["acc"] = _n(acc)
    return got


@pytest.mark.parametrize("S", P.WIDE_S)
def test_wide_blend_probes_exact(hip_lib, S):
    """Every residue of the forward's `s, s + 4, s += 8` loop and its tail; quads of the backward that straddle two rays and
    a ragged last quad (R = 3 with S % 4 != 0)."""
    for R in P.WIDE_R:
        for C in P.WIDE_C:
            p = P.blend_wide_probe(R, S, C)
            P.check_blend(p, run_blend_wide(p), f"wide S={S} R={R} C={C}", wide=True)


def test_wide_blend_backward_at_the_workgroup_cap(hip_lib):
    """R S = 528771 samples at C = 1: more quads than 16384 workgroups take in one pass, so the grid-stride loop runs."""
    R, S, C = P.WIDE_CAP
    p = P.blend_wide_probe(R, S, C)
    P.check_blend(p, run_blend_wide(p), f"wide cap R={R} S={S} C={C}", wide=True)


def run_epilogue(p):
    from emernerf_amd import ops
    st, acc, sky = _d(p["stats"], True), _d(p["acc"], True), _d(p["sky"], True)
    opa, dep, med, rgb = ops.ray_epilogue(st, acc, sky)
    ((opa * _d(p["d_opa"])).sum() + (dep * _d(p["d_dep"])).sum() + (rgb * _d(p["d_out"])).sum()).backward()
    return dict(opacity=_n(opa)[:, 0], depth=_n(dep)[:, 0], median=_n(med)[:, 0], rgb=_n(rgb), d_stats=_n(st.grad), d_acc=_n(acc.grad),
                d_sky=_n(sky.grad))


def test_epilogue_probe(hip_lib):
    """sum w on 0, 1e-6f and its neighbours, 1 and its upper neighbour: the clamp and its gradient mask exactly."""
    p = P.epilogue_probe()
    P.check_epilogue_probe(p, run_epilogue(p), "epilogue")


# --------------------------------------------------------------------------------------------------- realistic inputs
def _report(rep, what):
    short = {(k[len(what) + 1:] if k.startswith(what) else k): v for k, v in rep.items()}
    print(f"\n[worst err / bound] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in short.items()))


@pytest.mark.parametrize("R,S", P.REAL_SHAPES)
def test_realistic_rays_inside_the_bounds(hip_lib, R, S):
    """Sorted edges in [0.1, 50], sigma = rand^3 * 2, one all-zero and one saturated ray.  Every entry inside its bound, the
    median exact (no ray of these seeds has a cumsum of w within its bound of 0.5: test_composite_bounds_cpu.py), and
    composite_rgb against the fp64 restatement itself.  Measured on an MI355X: DESIGN.md 4.4."""
    p = P.realistic(R, S)
    rep = {}
    what = f"R={R} S={S}"
    got = run_render(p)
    P.check_real_render(p, got, what, rep)
    fused = run_composite(p)
    P.check_real_composite(p, fused, what + " fused", rep, wsum=got["stats"][:, 0])
    assert np.array_equal(fused["weights"], got["weights"]) and np.array_equal(fused["trans"], got["trans"])
    _report(rep, what)


@pytest.mark.parametrize("C", [None, 1, 3, 6, 9, 64, 100])
def test_realistic_accumulate_and_blends_inside_the_bounds(hip_lib, C):
    rng = np.random.default_rng(7)
    R, S = 5, 130
    p = dict(w=rng.random((R, S)).astype(np.float32), v=None if C is None else rng.standard_normal((R, S, C)).astype(np.float32),
             go=rng.standard_normal((R, C or 1)).astype(np.float32))
    rep = {}
    P.check_real_accumulate(p, *run_accumulate(p), f"accumulate C={C}", rep)
    if C in (3, 64, 100):
        q = P.realistic_blend(R, S, None if C == 3 else C)
        P.check_real_blend(q, run_blend(q) if C == 3 else run_blend_wide(q), f"blend C={C}", wide=C != 3, report=rep)
    _report(rep, f"C={C}")


def test_device_expf_error_is_inside_E_EXPF(hip_lib):
    """The bounds' one measured constant, kept honest: through render_weights itself (S = 2, dt = 1, sigma_1 = 0:
    trans[:, 1] = expf(-sigma_0)), a million arguments in [0, 100] against float64 exp of the fp32 argument.  E_EXPF is the
    measured maximum rounded up plus one ulp of margin, so the maximum seen here must stay at or below E_EXPF - 1."""
    from emernerf_amd import ops
    from tests import _bounds as B
    rng = np.random.default_rng(0)
    xs = np.concatenate([np.linspace(0, 100, 1 << 19), rng.random(1 << 19) * 100, rng.random(1 << 18) * 2,
                         np.arange(0, 100.25, 0.25)]).astype(np.float32)
    ts = np.zeros((xs.size, 2), np.float32)
    ts[:, 1] = 1
    sg = np.zeros((xs.size, 2), np.float32)
    sg[:, 0] = xs
    T = _n(ops.render_weights(_d(ts), _d(ts + 1), _d(sg))[1])
    assert (T[:, 0] == 1).all()
    ref = np.exp(-xs.astype(np.float64))
    normal = ref >= 2.0 ** -126
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    err = np.abs(T[:, 1].astype(np.float64) - ref)
    worst = float((err[normal] / ulp[normal]).max())
    print(f"\n[expf] worst error {worst:.3f} ulp over {int(normal.sum())} arguments (E_EXPF = {B.E_EXPF:g}); below the normal range: "
          f"{float(err[~normal].max()):.3e} absolute")
    assert worst <= B.E_EXPF - 1.0
    assert float(err[~normal].max()) <= B.TINY


# ------------------------------------------------------------------------------- what the shared stages rely on
@pytest.mark.parametrize("R,S", [(5, 1), (5, 65), (13, 129)])
def test_optional_pointers_do_not_change_the_other_results(hip_lib, R, S):
    """The scan kernels share one chunk function, one ray-statistics accumulator and one reverse chunk whatever the caller asks
    for, so through the C entry points: every output of emer_render_weights_fwd / emer_composite_rgb_fwd is bitwise the same with
    the other optional outputs requested as with them null, and d_sigma of both backwards is bitwise the same with an upstream
    pointer null as with it pointing at zeros."""
    from emernerf_amd import _lib
    from emernerf_amd.ops import _ptr, _stream
    p = {k: _d(v) for k, v in P.realistic(R, S).items()}
    ts, te, sg, st = p["ts"], p["te"], p["sg"], _stream(p["sg"])
    new = lambda *shape: torch.full(shape, 7.5, device=DEV)  # noqa: E731

    def render_fwd(want):
        o = {k: (new(R, S + 1) if k == "cdfs" else new(R, 4) if k == "ray_stats" else new(R, S)) if k in want else None
             for k in ("weights", "trans", "alphas", "cdfs", "ray_stats", "t_mid", "t_dist")}
        _lib.call("emer_render_weights_fwd", _ptr(ts), _ptr(te), _ptr(sg), R, S, *(_ptr(o[k]) for k in o), st)
        return o

    full = render_fwd(("weights", "trans", "alphas", "cdfs", "ray_stats", "t_mid", "t_dist"))
    for k in full:
        assert torch.equal(render_fwd((k,))[k], full[k]), f"render_weights_fwd: {k} alone differs from {k} among all outputs"

    need = ("weights", "ray_stats", "opacity", "depth")
    shapes = dict(weights=(R, S), trans=(R, S), t_mid=(R, S), t_dist=(R, S), ray_stats=(R, 4), opacity=(R,), depth=(R,), median_depth=(R,), rgb_out=(R, 3))

    def composite_fwd(want):
        o = {k: new(*shape) if (k in want or k in need) else None for k, shape in shapes.items()}
        _lib.call("emer_composite_rgb_fwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), _ptr(p["sky"]), R, S, *(_ptr(o[k]) for k in o), st)
        return o

    cfull = composite_fwd(tuple(shapes))
    for k in ("trans", "t_mid", "t_dist", "median_depth", "rgb_out"):
        got = composite_fwd((k,))
        for name in need + (k,):
            assert torch.equal(got[name], cfull[name]), f"composite_rgb_fwd: {name} with only {k} requested differs"
    got = composite_fwd(())
    for name in need:
        assert torch.equal(got[name], cfull[name]), f"composite_rgb_fwd: {name} with no optional output differs"

    ups = dict(d_weights=p["dW"], d_trans=p["dT"], d_alphas=p["dA"], d_ray_stats=p["dS"])

    def render_bwd(g):
        ds = new(R, S)
        _lib.call("emer_render_weights_bwd", _ptr(ts), _ptr(te), _ptr(sg), *(_ptr(g[k]) for k in ups), R, S, _ptr(ds), st)
        return ds

    for k in ups:
        assert torch.equal(render_bwd({**ups, k: None}), render_bwd({**ups, k: torch.zeros_like(ups[k])})), f"render_weights_bwd: {k} null vs zeros"

    cups = dict(d_rgb_out=p["d_out"], d_opacity=p["d_opa"], d_depth=p["d_dep"], d_weights=p["dW"], d_trans=p["dT"])

    def composite_bwd(g):
        ds = new(R, S)
        _lib.call("emer_composite_rgb_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), _ptr(p["sky"]), _ptr(cfull["weights"]), _ptr(cfull["ray_stats"]),
                  *(_ptr(g[k]) for k in cups), R, S, _ptr(ds), None, None, st)
        return ds

    for k in cups:
        assert torch.equal(composite_bwd({**cups, k: None}), composite_bwd({**cups, k: torch.zeros_like(cups[k])})), f"composite_rgb_bwd: {k} null vs zeros"


# -------------------------------------------------------------------------------------------------- argument contract
def test_backward_beyond_4096_samples_is_refused_before_any_launch(hip_lib):
    """chunk_base holds 64 chunks: S = 4097 is an EmerError from both backward entry points, and d_sigma is not touched."""
    from emernerf_amd import _lib
    from emernerf_amd.ops import _ptr, _stream
    R, S = 2, 4097
    ts, te, sg = torch.zeros(R, S, device=DEV), torch.ones(R, S, device=DEV), torch.zeros(R, S, device=DEV)
    gw = torch.ones(R, S, device=DEV)
    ds = torch.full((R, S), 7.5, device=DEV)
    with pytest.raises(_lib.EmerError, match="S <= 4096"):
        _lib.call("emer_render_weights_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(gw), None, None, None, R, S, _ptr(ds), _stream(sg))
    w, st = torch.zeros(R, S, device=DEV), torch.zeros(R, 4, device=DEV)
    with pytest.raises(_lib.EmerError, match="S <= 4096"):
        _lib.call("emer_composite_rgb_bwd", _ptr(ts), _ptr(te), _ptr(sg), None, None, _ptr(w), _ptr(st), None, None, None, _ptr(gw), None,
                  R, S, _ptr(ds), None, None, _stream(sg))
    torch.cuda.synchronize()
    assert bool((ds == 7.5).all()), "a refused call wrote to d_sigma"
    # through the wrappers: the forward has no limit, the backward raises the same error
    from emernerf_amd import ops
    sgr = sg.clone().requires_grad_(True)
    out = ops.render_weights(ts, te, sgr)
    assert out[0].shape == (R, S)
    with pytest.raises(_lib.EmerError, match="S <= 4096"):
        out[0].sum().backward()


def test_accumulate_without_values_needs_one_channel(hip_lib):
    from emernerf_amd import _lib
    from emernerf_amd.ops import _ptr, _stream
    R, S = 3, 10
    w = torch.ones(R, S, device=DEV)
    out, go, dw = torch.full((R, 3), 7.5, device=DEV), torch.ones(R, 3, device=DEV), torch.full((R, S), 7.5, device=DEV)
    with pytest.raises(_lib.EmerError, match="n_channels == 1"):
        _lib.call("emer_accumulate_fwd", _ptr(w), None, R, S, 3, _ptr(out), _stream(w))
    with pytest.raises(_lib.EmerError, match="n_channels == 1"):
        _lib.call("emer_accumulate_bwd", _ptr(w), None, _ptr(go), R, S, 3, _ptr(dw), None, _stream(w))
    torch.cuda.synchronize()
    assert bool((out == 7.5).all()) and bool((dw == 7.5).all()), "a refused call wrote to its outputs"
