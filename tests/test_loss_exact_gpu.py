"""pixel_loss, lidar_loss, reg_losses / reg_losses6 (csrc/rayloss.hip) and emer_reduce_sum (csrc/proploss.hip) held to
exact probes and per-entry fp64 bounds (tests/_loss_probe.py has the restatements, the builders and the numpy models;
tests/test_loss_bounds_cpu.py shows what the probes catch).

* exact probes: dyadic inputs on which the kernel must equal the fp64 restatement rounded to fp32 as numbers (the sign of a
  zero is not held) -- values, per-ray buffers / block partials and gradients, through the C entry points (buffers pre-filled
  with NaN: an entry a launch does not write shows) and through the ops wrappers;
* realistic families: every entry inside its first-order bound (tests/_bounds.py pixel_bounds, lidar_bounds,
  reg_partial_bound), none excluded; every total is the double sum of the launch's own per-ray (per-block) values rounded once;
* the device logf stays inside E_LOGF - 1;
* pinned behaviours: a lidar batch without a valid ray / without a gt > 0 ray, reduce_sum at n = 0, the argument contracts.
"""
import numpy as np
import pytest
import torch

from tests import _loss_probe as P
from tests._bounds import E_LOGF, assert_err_bound, pixel_bounds

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = np.float32, np.float64
NAN = float("nan")


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, F32))).to(DEV)


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def _call(name, *args):
    from emernerf_amd import _lib
    from emernerf_amd.ops import _ptr
    _lib.call(name, *[_ptr(a) if isinstance(a, torch.Tensor) else a for a in args], _stream())
    torch.cuda.synchronize()


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _bitwise(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def _assert_total(total, parts, what, base=0.0):
    want = F32(np.asarray(parts, F32).astype(F64).sum() + float(base))
    assert F32(total) == want, f"{what}: total {float(total)!r} is not the double sum of the launch's own values rounded once ({float(want)!r})"


# ------------------------------------------------------------------------------------------------------------- reduce
def _reduce(x, accumulate, init):
    xd = _d(x) if len(x) else None
    out = torch.full((1,), float(init), device=DEV)
    _call("emer_reduce_sum", xd, len(x), int(accumulate), out)
    return float(out[0])


@pytest.mark.parametrize("n", P.REDUCE_N)
def test_reduce_sum_probes_exact(hip_lib, n):
    """Integers: the sum is exact in any order.  n = 0 writes 0 and, with accumulate, leaves out as it was."""
    b = P.build_reduce(n)
    assert _reduce(b["x"], 0, b["prev"]) == P.restate_reduce(b["x"], b["prev"], 0), f"n={n}"
    assert _reduce(b["x"], 1, b["prev"]) == P.restate_reduce(b["x"], b["prev"], 1), f"n={n} accumulate"
    if n == 0:
        assert _reduce(b["x"], 0, 3.25) == 0.0 and _reduce(b["x"], 1, 3.25) == 3.25


# -------------------------------------------------------------------------------------------------------------- pixel
def _pixel_launch(b, want=("rgb", "opa")):
    """emer_pixel_loss_fwd / _bwd as ops.pixel_loss calls them: (loss_rays, total, d_rgb, d_opacity) as numpy."""
    R = b["R"]
    rgb, pix, opa, sky = _d(b["rgb"]), _d(b["pix"]), _d(b["opa"]), _d(b["sky"])
    rays, loss = torch.full((R,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
    _call("emer_pixel_loss_fwd", rgb, pix, opa, sky, R, float(b["w_rgb"]), float(b["w_sky"]), rays, loss)
    up = torch.full((1,), b["up"], device=DEV)
    dr = torch.full((R, 3), NAN, device=DEV) if rgb is not None and "rgb" in want else None
    do = torch.full((R,), NAN, device=DEV) if opa is not None and "opa" in want else None
    _call("emer_pixel_loss_bwd", rgb, pix, opa, sky, R, float(b["w_rgb"]) * float(b["grad_scale"]), float(b["w_sky"]) * float(b["grad_scale"]),
          up, dr, do)
    return _n(rays), float(loss[0]), _n(dr), _n(do)


def _pixel_wrapper(b, want=("rgb", "opa")):
    from emernerf_amd import ops
    rd = _d(b["rgb"]).requires_grad_("rgb" in want)
    od = None if b["opa"] is None else _d(b["opa"]).requires_grad_("opa" in want)
    loss = ops.pixel_loss(rd, od, _d(b["pix"]), _d(b["sky"]), b["w_rgb"], b["w_sky"], grad_scale=b["grad_scale"])
    (loss * b["up"]).backward()
    return float(loss), _n(rd.grad), None if od is None else _n(od.grad)


@pytest.mark.parametrize("mode", P.PIXEL_MODES)
@pytest.mark.parametrize("R", P.PIXEL_R)
def test_pixel_probes_exact(hip_lib, R, mode):
    """rgb-only (opacity = sky = None), sky-only (rgb = None) and both; upstream 2^-2 and grad_scale 2^5: the value does not
    carry grad_scale (it equals the restatement, which has none), both gradients do; d_rgb only and d_opacity only."""
    for seed in (0, 1):
        b = P.build_pixel(R, mode, seed)
        what = f"pixel {mode} R={R} seed={seed}"
        rays, total, dr, do = _pixel_launch(b)
        P.check_pixel_outputs(b, rays, total, dr, do, what)
        if mode != "sky":   # (the wrapper needs rgb)
            wl, wr, wo = _pixel_wrapper(b)
            assert wl == total and _bitwise(wr, dr) and (do is None or _bitwise(wo, do)), f"{what}: ops.pixel_loss differs from the entry points"
            wl1, wr1, wo1 = _pixel_wrapper(b, want=("rgb",))
            assert wl1 == total and _bitwise(wr1, dr) and wo1 is None, f"{what}: d_rgb only"
        if mode == "both":
            wl2, wr2, wo2 = _pixel_wrapper(b, want=("opa",))
            assert wl2 == total and wr2 is None and _bitwise(wo2, do), f"{what}: d_opacity only"
            _, _, dr3, do3 = _pixel_launch(b, want=("opa",))
            assert dr3 is None and _bitwise(do3, do)


@pytest.mark.parametrize("R", [257, 513])
def test_pixel_realistic_inside_the_bounds(hip_lib, R):
    """Measured on an MI355X, worst err / bound over both R: per-ray 0.23, d_rgb 0.14, d_opacity 0.38."""
    b = P.realistic_pixel(R)
    st, bd = b["ref"], pixel_bounds(b["ref"])
    rays, total, dr, do = _pixel_launch(b)
    for k, got in (("rays", rays), ("d_rgb", dr), ("d_opa", do)):
        assert_err_bound(got, st[k], bd[k], f"kernel pixel R={R} {k}")
    _assert_total(total, rays, f"pixel R={R}")
    wl, wr, wo = _pixel_wrapper(b)
    assert wl == total and _bitwise(wr, dr) and _bitwise(wo, do)


def _logf_sweep(n_log2):
    """2^n_log2 opacities in [1e-6, 1]: a quarter log-spaced from 1e-6, a quarter 1 - log-spaced down to 1 - 1e-7, an eighth each
    of uniform random, dense random in [1e-6, 1e-3] and in [0.999, 1], and a uniform grid.  _logf_sweep(23) is the set E_LOGF
    was measured on (tests/_bounds.py)."""
    n = 1 << (n_log2 - 2)
    rng = np.random.default_rng(5)
    o = np.concatenate([np.exp(np.linspace(np.log(1e-6), 0.0, n)), 1.0 - np.exp(np.linspace(np.log(1e-7), 0.0, n)), rng.random(n // 2),
                        rng.uniform(1e-6, 1e-3, n // 2), rng.uniform(0.999, 1.0, n // 2), np.linspace(1e-6, 1.0, n // 2)])
    return np.clip(np.clip(o, F32(1e-6), 1.0).astype(F32), F32(1e-6), F32(1.0))


def test_device_logf_error_is_inside_E_LOGF(hip_lib):
    """Sky-only pixel_loss at w_sky = 1, R = 2^20: loss_rays[r] = -logf(arg_r) / R exactly -- logf(o) with sky_mask = 0,
    logf(fl(1 - o)) with sky_mask = 1 -- against float64 log of the fp32 argument.  Fails above E_LOGF - 1 ulps."""
    o = _logf_sweep(20)
    R = o.size
    assert R == 1 << 20
    for sky in (0.0, 1.0):
        b = dict(R=R, rgb=None, pix=None, opa=o, sky=np.full(R, sky, F32), w_rgb=0.0, w_sky=1.0, up=1.0, grad_scale=1.0)
        rays, _, _, _ = _pixel_launch(b, want=())
        got = -(rays.astype(F64) * R)
        arg = o if sky == 0.0 else (F32(1.0) - o).astype(F32)
        keep = arg > 0
        assert (got[~keep] == -100.0).all(), "logf(0) is not clamped to -100"
        ref = np.log(arg[keep].astype(F64))
        ulp = np.spacing(np.abs(ref).astype(F32)).astype(F64)
        err = np.abs(got[keep] - ref) / ulp
        i = int(np.argmax(err))
        print(f"\n[logf] sky={sky:g}: worst {err[i]:.3f} ulp at arg {arg[keep][i]!r}; not correctly rounded {np.mean(got[keep] != ref.astype(F32)):.4f}")
        assert err[i] <= E_LOGF - 1.0, f"device logf is {err[i]:.3f} ulp off at {arg[keep][i]!r}: outside E_LOGF - 1 = {E_LOGF - 1.0}"


# -------------------------------------------------------------------------------------------------------------- lidar
def _lidar_launch(b, want_grads=True, **over):
    """emer_lidar_loss in one call: (loss_rays [R], counts [2], total, d_depth [R], d_weights [R, S])."""
    c = dict(b, **over)
    R, S = c["R"], c["S"]
    ws, loss = torch.full((R + 2,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
    dd = torch.full((R,), NAN, device=DEV) if want_grads else None
    dw = torch.full((R, S), NAN, device=DEV) if want_grads else None
    up = torch.full((1,), c["up"], device=DEV)
    _call("emer_lidar_loss", _d(c["depth"]), _d(c["gt"]), _d(c["w"]), _d(c["t"]), R, S, float(c["eps"]), float(c["max_depth"]), float(c["w_depth"]),
          float(c["w_sight"]), up, ws, loss, dd, dw)
    w = _n(ws)
    return w[:R], w[R:], float(loss[0]), _n(dd), _n(dw)


def _lidar_wrapper(b):
    from emernerf_amd import ops
    dd, wd = _d(b["depth"]).view(-1, 1).requires_grad_(True), _d(b["w"]).requires_grad_(True)
    loss = ops.lidar_loss(dd, wd, _d(b["gt"]).view(-1, 1), _d(b["t"]), b["eps"], b["max_depth"], b["w_depth"], b["w_sight"])
    (loss * b["up"]).backward()
    return float(loss), _n(dd.grad).reshape(-1), _n(wd.grad)


def _lidar_check(b, what, exact):
    rays, counts, total, dd, dw = _lidar_launch(b)
    assert counts[0] == b["ref"]["n_pos"] and counts[1] == b["ref"]["n_valid"], f"{what}: counts {counts} vs {b['ref']['n_pos']}, {b['ref']['n_valid']}"
    out = P.check_lidar_outputs(b, rays, total, dd, dw, what, exact=exact)
    wl, wdd, wdw = _lidar_wrapper(b)
    assert wl == total and _bitwise(wdd, dd) and _bitwise(wdw, dw), f"{what}: ops.lidar_loss differs from the entry point"
    return rays, total, dd, dw, out


@pytest.mark.parametrize("R,S,batch", P.LIDAR_CASES)
def test_lidar_probes_exact(hip_lib, R, S, batch):
    """Samples on gt - eps, gt + eps and one grid step on either side, in the first lanes, at lanes 62..65 and in the last
    chunk; gt on 0, 0.01f, max_depth and their neighbours; pred / max below 0, 0, 1, above 1; 1, 2 or 3 rays in the last
    workgroup; batches without a valid ray, without a gt > 0 ray, all valid, w_depth = 0, w_sight = 0."""
    for seed in (0, 1, 2, 3):
        b = P.build_lidar(R, S, batch, seed)
        _lidar_check(b, f"lidar {batch} R={R} S={S} seed={seed}", exact=True)


@pytest.mark.parametrize("R,S,eps,w_sight", P.LIDAR_REAL)
def test_lidar_realistic_inside_the_bounds(hip_lib, R, S, eps, w_sight):
    """Measured on an MI355X, worst err / bound over the 18 cases: per-ray 0.41, d_depth 0.49, d_weights 0.25."""
    b = P.realistic_lidar(R, S, eps, w_sight)
    _lidar_check(b, f"kernel lidar R={R} S={S} eps={eps} w_sight={w_sight:g}", exact=False)


def test_lidar_batch_without_a_valid_ray(hip_lib):
    """No ray with 0.01 < gt < max_depth: the reference returns NaN (the mean of an empty tensor, loss/base.py:60-72); the
    kernel returns a depth term of 0 and never divides by the valid count: a finite total, a depth gradient of exact zeros,
    and the sight term as it is without the depth term."""
    b = P.build_lidar(13, 65, "novalid", 0)
    assert b["ref"]["n_valid"] == 0 and np.isnan(b["ref"]["total_ref"])
    rays, total, dd, dw, _ = _lidar_check(b, "lidar no valid ray", exact=True)
    assert np.isfinite(total) and np.isfinite(rays).all() and (dd == 0).all()
    rays0, _, total0, _, dw0 = _lidar_launch(b, w_depth=0.0)
    assert total0 == total and _bitwise(rays0, rays) and _bitwise(dw0, dw) and total != 0.0


def test_lidar_batch_without_a_positive_range(hip_lib):
    """No ray with gt > 0: the mean[gt > 0] factor is 0: a sight term and weight gradients of exactly 0."""
    b = P.build_lidar(13, 65, "nopos", 0)
    assert b["ref"]["n_pos"] == 0 and b["ref"]["near"].any()
    rays, total, dd, dw, _ = _lidar_check(b, "lidar no gt > 0 ray", exact=True)
    assert (dw == 0).all() and total == 0.0 and (rays == 0).all() and (dd == 0).all()


# ---------------------------------------------------------------------------------------------------------------- reg
def _reg_forward(b):
    """emer_reg_losses_fwd / fwd6 directly: (block partials, total)."""
    T, c = b["T"], b["coefs"]
    g = lambda k: _d(T.get(k))  # noqa: E731
    n = lambda k: 0 if k not in T else int(T[k].size)  # noqa: E731
    ws, loss = torch.full((P.REG_MAX_BLOCKS,), NAN, device=DEV), torch.full((1,), NAN, device=DEV)
    base = None if b["base"] is None else torch.full((1,), b["base"], device=DEV)
    head = (g("dyn"), n("dyn"), float(c["dyn"]), g("shadow"), n("shadow"), float(c["shadow"]), g("feat"), g("feat_gt"), n("feat"), float(c["feat"]))
    if "flow2" in T:
        _call("emer_reg_losses_fwd6", *head, g("flow6"), g("flow2"), int(T["flow6"].shape[0]), float(c["cycle"]), base, ws, loss)
    else:
        _call("emer_reg_losses_fwd", *head, g("ff"), g("fpb"), g("bf"), g("bpf"), n("fpb"), float(c["cycle"]), base, ws, loss)
    blocks = P.reg_geometry(T)[0]
    w = _n(ws)
    assert np.isnan(w[blocks:]).all(), "the forward wrote past its block count"
    return w[:blocks], float(loss[0])


_KW = dict(dyn="dynamic_density", shadow="shadow_ratio", feat="feat", fpb="forward_pred_backward_flow", bpf="backward_pred_forward_flow")


def _reg_wrapper(b, need=None):
    """ops.reg_losses with upstream b['up']: (total, {name: gradient or None}, d_ff, d_base)."""
    from emernerf_amd import ops
    T, c = b["T"], b["coefs"]
    lv = {k: _d(v).requires_grad_(k != "feat_gt" and (need is None or k in need)) for k, v in T.items()}
    base = None if b["base"] is None else torch.full((), b["base"], device=DEV).requires_grad_(True)
    kw = {_KW[k]: lv[k] for k in ("dyn", "shadow", "feat") if k in lv}
    if "feat" in lv:
        kw["feat_gt"] = lv["feat_gt"]
    if "flow2" in lv:
        kw["flow_pair"] = (lv["flow6"], lv["flow2"])
    elif "fpb" in lv:
        kw.update(forward_flow=lv["ff"], forward_pred_backward_flow=lv["fpb"], backward_flow=lv["bf"], backward_pred_forward_flow=lv["bpf"])
    out = ops.reg_losses(base, c_dyn=c["dyn"], c_shadow=c["shadow"], c_feat=c["feat"], c_cycle=c["cycle"], grad_scale=b["grad_scale"], **kw)
    out.backward(torch.full((), b["up"], device=DEV))
    grads = {k: _n(lv[k].grad) for k in ("dyn", "shadow", "feat", "fpb", "bpf", "flow2") if k in lv}
    d_ff = next((_n(lv[k].grad) for k in ("ff", "bf", "flow6") if k in lv and lv[k].grad is not None), None)
    return float(out), grads, d_ff, None if base is None else float(base.grad)


@pytest.mark.parametrize("family", list(P.reg_families()))
def test_reg_probes_exact(hip_lib, family):
    """Single-term counts across the launch geometry (1024 elements per block, the 1024-block cap), the trainer's presence
    patterns, no base, and the packed form on the same numbers with values of their own in the blocks it must not read."""
    b = P.build_reg(**P.reg_families()[family])
    partials, total = _reg_forward(b)
    wl, grads, d_ff, d_base = _reg_wrapper(b)
    assert wl == total, f"reg {family}: ops.reg_losses returns another total"
    P.check_reg_outputs(b, partials, total, grads, f"reg {family}", d_ff, d_base)
    if len(grads) > 1:      # gradients requested for a subset only
        first = next(iter(grads))
        _, g1, _, _ = _reg_wrapper(b, need=(first,))
        assert _bitwise(g1[first], grads[first]) and all(v is None for k, v in g1.items() if k != first), f"reg {family}: subset of gradients"


REG_REAL_GPU = P.REG_REAL + [dict(R=1048577, S=1, E=1, terms="d"), dict(R=2097157, S=1, E=1, terms="d"), dict(R=87382, S=1, E=1, packed=True, terms="c")]


@pytest.mark.parametrize("kw", REG_REAL_GPU, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_reg_realistic_inside_the_bounds(hip_lib, kw):
    """Every block partial and gradient entry inside its bound; the packed form is held directly to fp64.  Measured on an
    MI355X, worst err / bound: block partials 0.11, d_dyn 0.20, d_shadow 0.12, d_feat 0.26, d_flow 0.31."""
    b = P.realistic_reg(**kw)
    partials, total = _reg_forward(b)
    wl, grads, d_ff, _ = _reg_wrapper(b)
    assert wl == total and d_ff is None
    P.check_reg_realistic(b, partials, total, grads, f"kernel reg {kw}")


# -------------------------------------------------------------------------------------------------- argument contracts
def test_argument_contracts_refuse_before_any_launch(hip_lib):
    """n_rays < 1, eps <= 0, max_depth <= 0, a missing companion pointer, a gradient requested for an absent term: EmerError,
    and no output buffer is touched."""
    from emernerf_amd import _lib
    x3, x1, x8 = torch.zeros((4, 3), device=DEV), torch.ones((4,), device=DEV), torch.ones((4, 8), device=DEV)
    out = [torch.full((16,), 7.5, device=DEV) for _ in range(4)]
    o0, o1, o2, o3 = out
    bad = [
        ("emer_pixel_loss_fwd", (x3, x3, x1, x1, 0, 1.0, 1.0, o0, o1)),                                   # n_rays < 1
        ("emer_pixel_loss_bwd", (x3, x3, x1, x1, 0, 1.0, 1.0, x1, o0, o1)),
        ("emer_pixel_loss_fwd", (x3, None, x1, x1, 4, 1.0, 1.0, o0, o1)),                                 # rgb without pixels
        ("emer_pixel_loss_fwd", (x3, x3, x1, None, 4, 1.0, 1.0, o0, o1)),                                 # opacity without sky_mask
        ("emer_pixel_loss_bwd", (None, None, x1, x1, 4, 1.0, 1.0, x1, o0, o1)),                           # d_rgb for an absent rgb term
        ("emer_pixel_loss_bwd", (x3, x3, None, None, 4, 1.0, 1.0, x1, o0, o1)),                           # d_opacity for an absent sky term
        ("emer_lidar_loss", (x1, x1, x8, x8, 0, 8, 2.0, 80.0, 1.0, 0.1, None, o0, o1, o2, o3)),           # n_rays < 1
        ("emer_lidar_loss", (x1, x1, x8, x8, 4, 0, 2.0, 80.0, 1.0, 0.1, None, o0, o1, o2, o3)),           # n_samples < 1
        ("emer_lidar_loss", (x1, x1, x8, x8, 4, 8, 0.0, 80.0, 1.0, 0.1, None, o0, o1, o2, o3)),           # eps <= 0
        ("emer_lidar_loss", (x1, x1, x8, x8, 4, 8, -1.0, 80.0, 1.0, 0.1, None, o0, o1, o2, o3)),
        ("emer_lidar_loss", (x1, x1, x8, x8, 4, 8, 2.0, 0.0, 1.0, 0.1, None, o0, o1, o2, o3)),            # max_depth <= 0
        ("emer_lidar_loss", (x1, x1, x8, None, 4, 8, 2.0, 80.0, 1.0, 0.1, None, o0, o1, o2, o3)),         # no t_vals
        ("emer_reg_losses_fwd", (None, 0, 0.0, None, 0, 0.0, x8, None, 32, 0.5, None, None, None, None, 0, 0.0, None, o0, o1)),     # feat without feat_gt
        ("emer_reg_losses_fwd", (x8, 0, 0.01, None, 0, 0.0, None, None, 0, 0.0, None, None, None, None, 0, 0.0, None, o0, o1)),     # count < 1
        ("emer_reg_losses_fwd", (None, 0, 0.0, None, 0, 0.0, None, None, 0, 0.0, x3, x3, None, x3, 12, 0.1, None, o0, o1)),         # cycle without bf
        ("emer_reg_losses_bwd", (x8, 32, 0.01, None, 0, 0.0, None, None, 0, 0.0, None, None, None, None, 0, 0.0, None, 1.0, None, None, o0, None, None)),  # d_feat, no feat
        ("emer_reg_losses_bwd", (x8, 32, 0.01, None, 0, 0.0, None, None, 0, 0.0, None, None, None, None, 0, 0.0, None, 1.0, None, None, None, o0, None)),  # d_fpb, no cycle
        ("emer_reg_losses_bwd6", (x8, 32, 0.01, None, 0, 0.0, None, None, 0, 0.0, None, None, 0, 0.0, None, 1.0, None, None, None, o0)),                   # d_flow2, no flow2
        ("emer_reg_losses_fwd6", (None, 0, 0.0, None, 0, 0.0, None, None, 0, 0.0, None, x8, 2, 0.1, None, o0, o1)),                                          # flow2 without flow6
    ]
    for name, args in bad:
        with pytest.raises(_lib.EmerError):
            _call(name, *args)
        torch.cuda.synchronize()
        assert all(bool((o == 7.5).all()) for o in out), f"{name}: a rejected call wrote to its outputs"
