"""The kernels that decide where every sample lands, on the device, against the exact probes, random families and fp32 models of
tests/_sample_probe.py (whose own power tests/test_sample_bounds_cpu.py shows without a GPU): emer_importance_sample in its three
output forms, emer_stot for all six maps, emer_ray_points, the fused emer_importance_sample_points up to its LDS capacity, the
two-launch fallback of PropNetEstimator.sampling above it, and the argument contracts.

The bar is bit equality: with the fp64 evaluation on the exact probes, with the model everywhere.  The one exception
is the ``log`` map, whose inverse is the device library's expf: it is held to exp, in fp64, of the model's bit-exact fp32
argument within ``P.LOG_ULP_DEVICE`` = 1.785 ulp (no document available to the project states the library's error,
so this is the largest error observed on an MI355X on the first run, 0.785 ulp over the 2 x 10^4 arguments of the random family
with the final rounding included, plus 1 ulp).

Every output sits between guards of sentinel NaNs that must come back with their bits and is handed over filled with the same
sentinel, so a write outside a row's range and an entry left unwritten both show.
"""
import numpy as np
import pytest
import torch

from tests import _sample_probe as P
from tests.test_update_exact_gpu import Guarded, _dev, _ptr, _stream, _t

pytestmark = pytest.mark.gpu

F32 = np.float32
FORMS = ("edges", "times", "intervals")


def _sample(b, form, points=None):
    """One emer_importance_sample (or, with points = (want_pos,), emer_importance_sample_points) on guarded outputs."""
    from emernerf_amd import _lib
    R, m = b["vals"].shape
    n = b["n"]
    vals, cdfs, jit = _t(b["vals"]), _t(b["cdfs"]), _t(b["jitter"])
    t_min, t_max, typ = b["stot"]
    s = Guarded(R * (n + 1))
    what = f"{b['name']} {form}"
    if points is not None:
        g = b["geo"]
        ts, te, normed = Guarded(R * n), Guarded(R * n), Guarded(R * n * 3)
        pos = Guarded(R * n * 3) if points[0] else None
        o, d, aabb = _t(g["o"]), _t(g["d"]), _t(g["aabb"])
        _lib.call("emer_importance_sample_points", _ptr(vals), _ptr(cdfs), R, m, n, _ptr(jit), _ptr(s.view), _ptr(ts.view), _ptr(te.view), float(t_min),
                  float(t_max), P.STOT_TYPES[typ], _ptr(o), _ptr(d), _ptr(aabb), int(g["unbounded"]), _ptr(normed.view), _ptr(None if pos is None else pos.view),
                  _stream())
        return dict(s=s.result(what).reshape(R, n + 1), ts=ts.result(what).reshape(R, n), te=te.result(what).reshape(R, n),
                    normed=normed.result(what).reshape(R, n, 3), pos=None if pos is None else pos.result(what).reshape(R, n, 3))
    t = Guarded(R * (n + 1)) if form == "times" else Guarded(R * n) if form == "intervals" else None
    te = Guarded(R * n) if form == "intervals" else None
    if form == "edges":         # the call of nerfacc_compat: no s -> t at all
        t_min, t_max, typ = 0.0, 1.0, "uniform"
    _lib.call("emer_importance_sample", _ptr(vals), _ptr(cdfs), R, m, n, _ptr(jit), _ptr(s.view), _ptr(None if t is None else t.view),
              _ptr(None if te is None else te.view), float(t_min), float(t_max), P.STOT_TYPES[typ], _stream())
    got = dict(s=s.result(what).reshape(R, n + 1))
    if form == "times":
        got["t"] = t.result(what).reshape(R, n + 1)
    if form == "intervals":
        got["ts"], got["te"] = t.result(what).reshape(R, n), te.result(what).reshape(R, n)
    return got


def _hold(b):
    for form in FORMS:
        P.check_sample(b, _sample(b, form), f"{b['name']} {form}")


# ------------------------------------------------------------------------------------------------------ emer_importance_sample
@pytest.mark.parametrize("m", [2, 3, 64, 65])
def test_sampler_dyadic_probes(hip_lib, m):
    """n + 1 in {2, 64, 128}, beta = 0.5 by default and a per-ray cycle of 0.25, 0, 0.5: bit for bit the fp64 result."""
    for n in (1, 63, 127):
        for jitter in ("default", "cycle"):
            _hold(P.build_dyadic(m, n, jitter))


def test_sampler_tie_threshold_and_end_clamp_probes(hip_lib):
    """u equal to interior CDF values and a run of three; brackets of width 2^-33, 2^-34 and 0, an all-equal CDF; u == c_last."""
    for b in (P.build_ties(), P.build_threshold(), P.build_end_clamp()):
        _hold(b)


# R in {1, 3, 4, 5, 37} (blocks of four rays: one partial, one full, one full + one ray, ten), m on both sides of the wave width and
# of the 48 KiB of LDS a launch gets without asking (m = 1536 | 1537) up to the ABI's 4096, n on both sides of 64 and 128
SAMPLER_RANDOM = [(1, 2, 1, "none"), (3, 3, 63, "uniform"), (4, 64, 64, "edge"), (5, 65, 127, "none"), (37, 129, 128, "uniform"), (5, 1536, 257, "edge"),
                  (4, 1537, 128, "uniform"), (5, 4096, 128, "edge"), (3, 4096, 1, "none"), (37, 2, 257, "uniform"), (5, 129, 64, "edge")]


@pytest.mark.parametrize("R,m,n,jitter", SAMPLER_RANDOM)
def test_sampler_random_families(hip_lib, R, m, n, jitter):
    """Peaky, half-flat, all-zero, one-bin and rescaled histograms in all three output forms, bit for bit the model; the edges
    are sorted and inside [v_0, v_last]."""
    b = P.build_random(R, m, n, jitter)
    for form in FORMS:
        got = _sample(b, form)
        P.check_sample(b, got, f"{b['name']} {form}")
        assert P.edges_sorted_and_inside(b, got["s"])


# ------------------------------------------------------------------------------------------------------------------ emer_stot
def _stot(b):
    from emernerf_amd import _lib
    s = _t(b["s"])
    out = Guarded(s.numel())
    _lib.call("emer_stot", _ptr(s), s.numel(), float(b["planes"][0]), float(b["planes"][1]), P.STOT_TYPES[b["typ"]], _ptr(out.view), _stream())
    return out.result(b["name"])


def test_stot_exact_probes(hip_lib):
    for b in P.build_stot_exact():
        P.check_stot(b, _stot(b), b["name"])


@pytest.mark.parametrize("typ", list(P.STOT_TYPES))
def test_stot_random_family(hip_lib, typ):
    """10^4 values of s (0, 1, 0.5 and its neighbours, a quarter of them around the break of the piecewise maps) with two plane
    pairs.  Five maps bit for bit; ``log`` within P.LOG_ULP_DEVICE of exp of the fp32 argument (the largest distance is printed;
    first run on an MI355X: 0.764 ulp for the planes (0.1, 1000), 0.785 ulp for (0.5, 300))."""
    for b in P.build_stot_random():
        if b["typ"] != typ:
            continue
        got = _stot(b)
        if typ == "log":
            worst = P.check_log(b["name"], got, b["arg"], P.LOG_ULP_DEVICE)
            exact = float((got.view(np.uint32) == b["want"].view(np.uint32)).mean())
            print(f"\n[log] device expf, {b['name']}: at most {worst:.3f} ulp from exp of the fp32 argument; {exact:.4f} of the results are the correctly rounded one")
        else:
            P.check_stot(b, got, b["name"])


# ------------------------------------------------------------------------------------------------------------ emer_ray_points
def _points(b, out_dim, want_pos):
    from emernerf_amd import _lib
    R, S = b["R"], b["S"]
    o, d, ts, te, aabb = (_t(b[k]) for k in ("o", "d", "ts", "te", "aabb"))
    times = _t(b["times"]) if out_dim == 4 else None
    normed, pos = Guarded(R * S * out_dim), (Guarded(R * S * 3) if want_pos else None)
    _lib.call("emer_ray_points", _ptr(o), _ptr(d), _ptr(ts), _ptr(te), _ptr(times), _ptr(aabb), int(b["unbounded"]), _ptr(normed.view), out_dim,
              _ptr(None if pos is None else pos.view), R, S, _stream())
    what = f"{b['name']} out_dim={out_dim}"
    return dict(normed=normed.result(what).reshape(R, S, out_dim), pos=None if pos is None else pos.result(what).reshape(R, S, 3))


@pytest.mark.parametrize("R,S", [(1, 1), (3, 64), (67, 128), (5, 257)])
@pytest.mark.parametrize("unbounded", [True, False])
def test_ray_points(hip_lib, R, S, unbounded):
    """Exact probes (points on a face, mag exactly 1, 2, 4, 8) against fp64 and the random family (far outside, both sides of
    mag = 1, a ray that ends at t = inf: NaN where the model has NaN) against the model: contracted points, the per-ray times
    column of out_dim = 4, world positions wanted or not."""
    for b in (P.build_points_exact(R, S, unbounded), P.build_points_random(R, S, unbounded)):
        for out_dim in (3, 4):
            for want_pos in (True, False):
                P.check_points(b, _points(b, out_dim, want_pos), f"{b['name']} out_dim={out_dim} pos={want_pos}", None, out_dim)


# ---------------------------------------------------------------------------------------------- emer_importance_sample_points
FUSED = [(m, n) for m in (2, 65, 129) for n in (1, 63, 64, 65, 128)]


@pytest.mark.parametrize("m,n", FUSED)
def test_fused_sampler_points_random_families(hip_lib, m, n):
    """Every output of the fused kernel bit for bit the MODEL (the sampler, the s -> t map, the points of the new intervals)."""
    for i, (R, jitter) in enumerate(((5, "uniform"), (37, "edge"), (4, "none"))):
        b = P.attach_geometry(P.build_random(R, m, n, jitter), unbounded=(i != 2))
        P.check_sample_points(b, _sample(b, "fused", points=(i != 1,)), f"fused {b['name']}")


def test_fused_sampler_points_on_the_probes(hip_lib):
    for src in (P.build_dyadic(65, 63, "cycle"), P.build_dyadic(2, 127, "default"), P.build_ties(), P.build_threshold(), P.build_end_clamp()):
        for unbounded in (True, False):
            b = P.attach_geometry(src, unbounded)
            P.check_sample_points(b, _sample(b, "fused", points=(True,)), f"fused {b['name']} unbounded={unbounded}")


def _capacity_case():
    from emernerf_amd import ops
    cap = ops.sample_points_capacity()
    m = 4096
    n = cap - 2 * m - 1
    if n < 1:
        n = 128
        m = (cap - n - 1) // 2
    assert 2 <= m <= 4096 and 2 * m + n + 1 == cap, (cap, m, n)
    return cap, m, n


def test_fused_sampler_points_exactly_at_capacity(hip_lib):
    """2 m + n + 1 == emer_importance_sample_points_capacity(): every float of the workgroup's LDS is in use."""
    cap, m, n = _capacity_case()
    b = P.attach_geometry(P.build_random(5, m, n, "edge"), True)
    P.check_sample_points(b, _sample(b, "fused", points=(True,)), f"fused at capacity {cap}: m={m} n={n}")


def test_fused_sampler_points_one_float_above_capacity_is_refused(hip_lib):
    from emernerf_amd import _lib
    cap, m, n = _capacity_case()
    b = P.attach_geometry(P.build_random(5, m, n + 1, "none"), True)
    with pytest.raises(_lib.EmerError, match="LDS"):
        _sample(b, "fused", points=(True,))


def test_prop_net_resamples_in_two_launches_above_capacity(hip_lib, monkeypatch):
    """PropNetEstimator.sampling with ray geometry: the proposal level (m = 2, n = 4095) fits and takes the fused kernel; the final
    round (m = 4096, n = capacity - 2 m: one float above) takes emer_importance_sample, its intervals carry no points, and its
    values are the model's for the CDF the level produced."""
    from emernerf_amd import _lib, ops
    from emernerf_amd.prop_net import PropNetEstimator
    cap, m, n = _capacity_case()
    assert m == 4096, "the device's LDS is smaller than the case was written for"
    n_final = n + 1
    dev = _dev()
    R = 5
    rng = np.random.default_rng(77)
    o, d = _t(P._f(rng.random((R, 3)) * 40)), _t(P._f(rng.standard_normal((R, 3))))
    d = torch.nn.functional.normalize(d, dim=-1)
    aabb = _t(P.AABB_TRAIN)
    planes = (0.1, 1000.0, "uniform_lindisp")
    seen, calls = {}, []
    real_call = _lib.call

    def spy(name, *a):
        calls.append(name)
        return real_call(name, *a)

    def sigma_fn(t0, t1):
        seen["t0"], seen["t1"] = t0, t1
        seen["points"] = getattr(t0, "_emer_points", None)
        seen["sigma"] = (1.0 + torch.sin(t0 * 0.37)) * 0.02
        return {"density": seen["sigma"][..., None]}

    monkeypatch.setattr(_lib, "call", spy)
    est = PropNetEstimator().to(dev)
    jit = _t(P._f(rng.random((2, R))))
    draws = iter(jit.unbind(0))
    est.jitter_fn = lambda n_rays, device: next(draws)
    t0, t1 = est.sampling([sigma_fn], [m - 1], n_final, R, planes[0], planes[1], planes[2], stratified=True,
                          ray_geometry=(o, d, [(aabb, True, False), (aabb, True, False)]))
    monkeypatch.setattr(_lib, "call", real_call)
    samplers = [c for c in calls if c.startswith("emer_importance_sample")]
    assert samplers == ["emer_importance_sample_points", "emer_importance_sample"], samplers
    assert seen["points"] is not None and getattr(t0, "_emer_points", None) is None
    unit = np.tile(np.array([0.0, 1.0], F32), (R, 1))
    lvl = dict(name="level", exact=False, vals=unit, cdfs=unit, n=m - 1, jitter=jit[0].cpu().numpy(), stot=planes)
    want = P.model_sample(lvl)
    P.same_bits("level starts", seen["t0"].cpu().numpy(), want["ts"])
    P.same_bits("level ends", seen["t1"].cpu().numpy(), want["te"])
    cdfs = ops.render_weights(seen["t0"], seen["t1"], seen["sigma"])[3].detach().cpu().numpy()
    assert cdfs.shape == (R, m)
    fin = dict(name="final", exact=False, vals=want["s"], cdfs=cdfs, n=n_final, jitter=jit[1].cpu().numpy(), stot=planes)
    want = P.model_sample(fin)
    P.same_bits("final starts", t0.cpu().numpy(), want["ts"])
    P.same_bits("final ends", t1.cpu().numpy(), want["te"])


# ---------------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts(hip_lib):
    """m = 1 and m = 4097, n = 0, an unknown transform type, t_ends without t_out: each is an EmerError before any launch.  R = 0
    returns without touching the outputs."""
    from emernerf_amd import _lib
    R, n = 3, 8
    buf = _t(np.tile(np.linspace(0.0, 1.0, 4097, dtype=F32), (R, 1)))
    jit = _t(np.full(R, 0.5, F32))
    geo = [_t(np.ones((R, 3), F32)), _t(np.ones((R, 3), F32)), _t(P.AABB_TRAIN)]
    outs = [Guarded(R * (n + 1)), Guarded(R * n), Guarded(R * n), Guarded(R * n * 3), Guarded(R * n * 3)]
    s, ts, te, normed, pos = (_ptr(x.view) for x in outs)

    def sampler(R=R, m=65, n=n, typ=1, t_out=ts, t_ends=te):
        _lib.call("emer_importance_sample", _ptr(buf), _ptr(buf), R, m, n, _ptr(jit), s, t_out, t_ends, 0.1, 1000.0, typ, _stream())

    def fused(R=R, m=65, n=n, typ=1):
        _lib.call("emer_importance_sample_points", _ptr(buf), _ptr(buf), R, m, n, _ptr(jit), s, ts, te, 0.1, 1000.0, typ, _ptr(geo[0]), _ptr(geo[1]),
                  _ptr(geo[2]), 1, normed, pos, _stream())

    for fn in (sampler, fused):
        for kw in (dict(m=1), dict(m=4097), dict(n=0), dict(typ=6), dict(typ=-1), dict(R=-1)):
            with pytest.raises(_lib.EmerError):
                fn(**kw)
        fn(R=0)
    with pytest.raises(_lib.EmerError, match="t_ends"):
        sampler(t_out=None)
    for typ in (6, -1):
        with pytest.raises(_lib.EmerError):
            _lib.call("emer_stot", _ptr(buf), 16, 0.1, 1000.0, typ, s, _stream())
    _lib.call("emer_stot", _ptr(buf), 0, 0.1, 1000.0, 1, s, _stream())
    with pytest.raises(_lib.EmerError):
        _lib.call("emer_ray_points", _ptr(geo[0]), _ptr(geo[1]), ts, te, None, _ptr(geo[2]), 1, normed, 4, None, R, n, _stream())      # out_dim 4 without times
    _lib.call("emer_ray_points", _ptr(geo[0]), _ptr(geo[1]), ts, te, None, _ptr(geo[2]), 1, normed, 3, pos, 0, n, _stream())
    torch.cuda.synchronize()
    for x in outs:
        assert P.is_sentinel(x.result("argument contracts")), "a refused or empty call wrote to its outputs"
