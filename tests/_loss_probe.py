"""Exact-arithmetic probes, numpy models and fp64 restatements of the loss kernels (test helper, not a test module).

``pixel_loss``, ``lidar_loss`` and ``reg_losses`` / ``reg_losses6`` (emernerf_amd/csrc/rayloss.hip) and the reduction
``emer_reduce_sum`` (csrc/proploss.hip) they share.

Restatements (``restate_*``): the reference's expressions written literally in fp64 on the fp32 inputs --
``F.mse_loss + w F.binary_cross_entropy`` (loss/base.py:83-185), ``DepthLoss("l2")`` + ``compute_line_of_sight_loss``
(loss/base.py:188-271, 430-464, with the scalar-mean x per-ray-mask product), the four mean-type regularisers, a plain sum.
What is an INTEGER fact is taken from the fp32 comparison the reference itself performs: the lidar band masks
``t < fl32(gt - fl32(eps))`` ..., the valid / gt > 0 masks, and whether fl32(pred / max) lies in [0, 1] (the clamp's gradient).
The floor of torch's BCE gradient is the fp32 constant 1e-12f.  Everything else is fp64.

Models (``model_*``): the kernels' own operation order in numpy, in fp32 (the emulation) or fp64: the per-ray expressions,
the per-lane strided sums of the lidar wave and the xor butterfly, the per-thread strided sums of reg_losses over
reg_blocks x 256 threads, wave butterfly, four wave partials, the finishing workgroup's double sum plus base, and
reduce_sum's 1024 strided double sums.  ``MUTANTS`` lists the one-line slips each model can be given.

Exact probes (``build_*``): dyadic inputs on which every intermediate is representable in fp32 and every sum stays below
2^24 units in any order, so a correct kernel equals the restatement rounded to fp32 entry by entry.  Each builder asserts
its preconditions in fp64.  A lidar sample in the near band ON gt has expf(-0) = 1: its delta is the fp32 `norm`, taken from
the kernel's correctly rounded fp32 chain eps / 3 -> sigma^2 -> sqrtf -> 1 / x, and the entry is held bit for bit
(``lidar_exact_flags``).  Two kinds of entry are held to their few-rounding bound of tests/_bounds.py instead: a near-band
sample OFF gt (a device expf of a non-zero argument), and a lidar quotient by an R / count that is no power of two.  What
decides a probe -- which band a sample on an edge falls into, which rays count, whether the clamp
passes a gradient, which elements a launch geometry reaches -- changes an entry by its whole value, not by roundings.
"""
import math

import numpy as np
import torch

from tests._head_probe import grid_of

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
BUDGET = 2.0 ** 24
EPS12 = F32(1e-12)          # torch's binary_cross_entropy_backward floor, as an fp32 constant
PI32 = F32(3.14159265358979323846)

# family -> {name: what it changes in the model}
MUTANTS = {
    "pixel": {
        "mean3R": "rgb term: mean over R for 3 R",
        "target": "BCE target sky for 1 - sky",
        "noclamp": "the -100 clamp of the logs dropped",
        "nofloor": "the 1e-12 floor of the BCE gradient dropped",
        "gs_value": "grad_scale folded into the value",
        "gs_dopa": "grad_scale missing from d_opacity",
        "no_up": "upstream gradient not applied",
    },
    "lidar": {
        "le_empty": "empty band t <= gt - eps",
        "le_near_lo": "near band t >= gt - eps",
        "le_near_hi": "near band t <= gt + eps",
        "far": "the far band t > gt + eps counted (w^2)",
        "valid_ge": "valid mask gt >= 0.01",
        "valid_le": "valid mask gt <= max_depth",
        "clamp_strict": "clamp gradient strict at the bounds",
        "clamp_pass": "clamp gradient passed outside [0, 1]",
        "mean_npos": "depth mean over the gt > 0 count for the valid count",
        "mean_R": "depth mean over R for the valid count",
        "no_posfactor": "the mean[gt > 0] factor dropped",
        "posfactor_per_ray": "the mean[gt > 0] factor applied per ray",
        "sigma_eps": "sigma = eps for eps / 3",
        "norm_pi": "pi cut to 3.14159 in norm",
        "norm_rsqrt": "norm by an approximate reciprocal square root (one ulp off)",
        "tail_lanes": "lanes of the last, partial 64-sample chunk dropped",
        "first64": "samples beyond the first 64 dropped",
        "skip_nonpos": "a ray with gt <= 0 skipped entirely",
    },
    "reg": {
        "divisor": "a term divided by another term's count",
        "cycle_second": "the cycle term's second square dropped",
        "swap_blocks": "packed: the predicted flows read from the other column blocks",
        "second_half": "packed: the second half read from the first",
        "unread_nonzero": "packed: the unread blocks of the gradient not zeroed",
        "grad_detached": "a gradient to the detached flows",
        "one_sweep": "elements past one grid sweep dropped",
        "tail": "the strided tail (last, partial sweep) dropped",
        "base_scaled": "base's gradient scaled by grad_scale",
    },
    "reduce": {
        "tail1024": "elements past the first 1024 dropped",
        "no_accumulate": "accumulate ignored",
    },
}
# Mutants that provably cannot show on any input (none was found for these kernels: every listed slip changes an entry).
EQUIVALENT = {}


def _exact32(a):
    a = np.asarray(a, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.array_equal(a.astype(F32).astype(F64), a))


def _is_exact32(a):
    a = np.asarray(a, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        return a.astype(F32).astype(F64) == a


def _pow2(n):
    n = int(n)
    return n >= 1 and (n & (n - 1)) == 0


def _cf(dt):
    """How a host float reaches a kernel: as a c_float in the fp32 emulation, unrounded in the fp64 model."""
    return (lambda v: F32(v)) if dt is F32 else (lambda v: F64(v))


# ------------------------------------------------------------------------------------------------------------- reduce
def restate_reduce(x, prev=0.0, accumulate=0):
    return float(np.asarray(x, F64).sum() + (float(prev) if accumulate else 0.0))


def model_reduce(x, prev=0.0, accumulate=0, mut=""):
    """reduce_sum_kernel: 1024 strided double sums, the xor butterfly inside each of the 16 waves, the 16 wave partials in
    order, + the previous value, one rounding to fp32."""
    x = np.asarray(x, F32).astype(F64).reshape(-1)
    if mut == "tail1024":
        x = x[:1024]
    pad = (-x.size) % 1024
    part = np.concatenate([x, np.zeros(pad)]).reshape(-1, 1024)
    acc = np.zeros(1024)
    for row in part:
        acc = acc + row
    acc = acc.reshape(16, 64)
    lanes = np.arange(64)
    off = 32
    while off:
        acc = acc + acc[:, lanes ^ off]
        off >>= 1
    t = 0.0
    for i in range(16):
        t += acc[i, 0]
    if accumulate and mut != "no_accumulate":
        t += float(prev)
    return F32(t)


REDUCE_N = (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000)


def build_reduce(n, seed=0):
    """Integers in [-8, 8] and an integer previous value: every partial sum in any order is exact."""
    rng = np.random.default_rng(100 * seed + n)
    return dict(x=rng.integers(-8, 9, n).astype(F32), prev=float(rng.integers(-40, 41)) + 0.5)


# -------------------------------------------------------------------------------------------------------------- pixel
def restate_pixel(rgb, pix, opa, sky, w_rgb, w_sky, up=1.0, grad_scale=1.0):
    """w_rgb F.mse_loss(rgb, pix) + w_sky F.binary_cross_entropy(opa, 1 - sky) in fp64 (a term whose tensors are None is
    absent): per-ray shares ``rays``, ``total``, the gradients times up grad_scale, and the parts the bounds need.  The value
    does NOT carry grad_scale."""
    R = (rgb if rgb is not None else opa).shape[0]
    rays = np.zeros(R)
    st = dict(R=R, w_rgb=float(w_rgb), w_sky=float(w_sky), d_rgb=None, d_opa=None, rgb_term=np.zeros(R), sky_term=np.zeros(R))
    k = float(up) * float(grad_scale)
    if rgb is not None:
        d = np.asarray(rgb, F64).reshape(R, 3) - np.asarray(pix, F64).reshape(R, 3)
        st["rgb_term"] = w_rgb * (d * d).sum(1) / (3 * R)
        st["d_rgb"] = k * w_rgb * 2.0 * d / (3 * R)
    if opa is not None:
        o, t = np.asarray(opa, F64).reshape(R), 1.0 - np.asarray(sky, F64).reshape(R)
        with np.errstate(divide="ignore"):
            lo, l1 = np.log(o), np.log(1.0 - o)
        A, B = t * np.maximum(lo, -100.0), (1.0 - t) * np.maximum(l1, -100.0)
        st.update(o=o, t=t, log_o=lo, log_1mo=l1, A=A, B=B)
        st["sky_term"] = w_sky * (-(A + B)) / R
        st["d_opa"] = k * w_sky * (o - t) / np.maximum(o * (1.0 - o), float(EPS12)) / R
    st["rays"] = st["rgb_term"] + st["sky_term"]
    st["total"] = float(st["rays"].sum())
    return st


def model_pixel(rgb, pix, opa, sky, w_rgb, w_sky, up=1.0, grad_scale=1.0, dt=F32, mut="", want=("rgb", "opa")):
    """pixel_loss_fwd/bwd_kernel as ops.pixel_loss calls them: the forward takes (w_rgb, w_sky), the backward
    (w_rgb grad_scale, w_sky grad_scale) -- the products formed on the host in double -- and the upstream scalar."""
    cf = _cf(dt)
    R = (rgb if rgb is not None else opa).shape[0]
    Rf = dt(R)
    gv = float(grad_scale) if mut == "gs_value" else 1.0
    wr, wk = cf(float(w_rgb) * gv), cf(float(w_sky) * gv)
    wrb, wkb = cf(float(w_rgb) * float(grad_scale)), cf(float(w_sky) * (1.0 if mut == "gs_dopa" else float(grad_scale)))
    upf = dt(1.0 if mut == "no_up" else up)
    l = np.zeros(R, dt)
    out = dict(d_rgb=None, d_opa=None)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if rgb is not None:
            d = np.asarray(rgb, dt).reshape(R, 3) - np.asarray(pix, dt).reshape(R, 3)
            s = np.zeros(R, dt)
            for c in range(3):
                s = s + d[:, c] * d[:, c]
            l = l + wr * s / (Rf if mut == "mean3R" else dt(3) * Rf)
            if "rgb" in want:
                out["d_rgb"] = upf * wrb * dt(2) * d / (dt(3) * Rf)
        if opa is not None:
            o = np.asarray(opa, dt).reshape(R)
            sk = np.asarray(sky, dt).reshape(R)
            t = sk if mut == "target" else dt(1) - sk
            lo, l1 = np.log(o), np.log(dt(1) - o)
            if mut != "noclamp":
                lo, l1 = np.maximum(lo, dt(-100)), np.maximum(l1, dt(-100))
            bce = -(t * lo + (dt(1) - t) * l1)
            l = l + wk * bce / Rf
            if "opa" in want:
                den = o * (dt(1) - o)
                if mut != "nofloor":
                    den = np.maximum(den, dt(EPS12))
                out["d_opa"] = upf * wkb * (o - t) / den / Rf
    out["rays"] = l.astype(dt)
    out["total"] = model_reduce(l) if dt is F32 else F64(l.sum())
    return out


PIXEL_R = (1, 2, 255, 256, 257, 513)
PIXEL_MODES = ("rgb", "sky", "both")


def build_pixel(R, mode, seed=0):
    """rgb / pixels on multiples of 2^-4; w_rgb = 3 2^-4 at R a power of two, 3 R 2^-4 otherwise, so w_rgb s / (3 R) is exact;
    opacity and sky on the four corners (1, 0), (0, 1) -> 0 and (1, 1), (0, 0) -> 100 (through the -100 clamp and 0 (-100));
    w_sky = 2^-6 (R a power of two) or R 2^-6; upstream 2^-2 and grad_scale 2^5: powers of two other than 1 that differ."""
    rng = np.random.default_rng(1000 * seed + R)
    p2 = _pow2(R)
    b = dict(R=R, mode=mode, up=2.0 ** -2, grad_scale=2.0 ** 5, rgb=None, pix=None, opa=None, sky=None, w_rgb=0.0, w_sky=0.0, pow2=p2)
    if mode in ("rgb", "both"):
        b["rgb"] = (rng.integers(0, 17, (R, 3)) / 16.0).astype(F32)
        b["pix"] = (rng.integers(0, 17, (R, 3)) / 16.0).astype(F32)
        b["w_rgb"] = (3.0 if p2 else 3.0 * R) * 2.0 ** -4
    if mode in ("sky", "both"):
        corner = (np.arange(R) + seed) % 4
        b["opa"] = np.array([1.0, 0.0, 1.0, 0.0], F32)[corner]
        b["sky"] = np.array([0.0, 1.0, 1.0, 0.0], F32)[corner]
        b["w_sky"] = (1.0 if p2 else float(R)) * 2.0 ** -6
    st = restate_pixel(b["rgb"], b["pix"], b["opa"], b["sky"], b["w_rgb"], b["w_sky"], b["up"], b["grad_scale"])
    assert _exact32(st["rays"]) and _exact32(st["total"]) and _exact32(b["w_rgb"]) and _exact32(b["w_sky"]), "pixel probe broken: value not exact"
    assert float(np.abs(st["rays"]).sum() * 2.0 ** grid_of(st["rays"])) < BUDGET, "pixel probe broken: the total is not exact in any order"
    if st["d_rgb"] is not None:
        assert _exact32(st["d_rgb"]), "pixel probe broken: d_rgb not exact"
    if st["d_opa"] is not None:
        want = np.where(b["opa"] == b["sky"], np.where(b["opa"] == 1, 1.0, -1.0), 0.0) * b["up"] * b["grad_scale"] * b["w_sky"] / float(EPS12) / R
        assert np.array_equal(st["d_opa"], want), "pixel probe broken: the corner gradients are not +-1 / 1e-12f / R"
        assert R < 4 or ((st["sky_term"] > 0).any() and (st["sky_term"] == 0).any())
    b["ref"] = st
    return b


def check_pixel_outputs(b, rays, total, d_rgb, d_opa, what):
    """Values, per-ray buffer and d_rgb equal the restatement as numbers.  d_opacity: exactly 0 on the (1, 0) / (0, 1) corners;
    on the others +-up w / 1e-12f / R: an exact numerator and two correctly rounded fp32 divisions, which fix it bit for bit at
    every R (where R is a power of two the second is exact and the value is the restatement rounded once)."""
    st = b["ref"]
    assert np.array_equal(np.asarray(rays, F64), st["rays"]), f"{what}: per-ray values differ from the restatement"
    assert float(total) == st["total"], f"{what}: total {float(total)!r} vs {st['total']!r}"
    if d_rgb is not None:
        assert np.array_equal(np.asarray(d_rgb, F64).reshape(-1, 3), st["d_rgb"]), f"{what}: d_rgb differs from the restatement"
    if d_opa is not None:
        got = np.asarray(d_opa, F64).reshape(-1)
        k = b["up"] * b["w_sky"] * b["grad_scale"] * (st["o"] - st["t"])
        assert _exact32(k), "pixel probe broken: up w (o - t) not exact"
        with np.errstate(over="ignore"):
            want = ((k.astype(F32) / EPS12).astype(F32) / F32(b["R"])).astype(F32)
            if b["pow2"]:
                assert np.array_equal(want, st["d_opa"].astype(F32))
        assert np.array_equal(got, want.astype(F64)), f"{what}: d_opacity differs: {got[:8]} vs {want[:8]}"


def realistic_pixel(R, seed=0):
    """opacity = clamp(rand^3 1.2, 1e-6, 1) (mass at both clamp ends), sky fraction 0.3, w_sky = 0.001, grad_scale = 1024."""
    g = torch.Generator().manual_seed(977 * seed + R)
    rgb, pix = torch.rand(R, 3, generator=g), torch.rand(R, 3, generator=g)
    opa = (torch.rand(R, generator=g) ** 3 * 1.2).clamp(1e-6, 1.0)
    sky = (torch.rand(R, generator=g) < 0.3).float()
    b = dict(R=R, rgb=rgb.numpy(), pix=pix.numpy(), opa=opa.numpy(), sky=sky.numpy(), w_rgb=1.0, w_sky=0.001, up=1.0, grad_scale=1024.0)
    b["ref"] = restate_pixel(b["rgb"], b["pix"], b["opa"], b["sky"], 1.0, 0.001, 1.0, 1024.0)
    return b


def ref_pixel_torch(b, dtype=torch.float32):
    """The reference's own evaluation by torch on the CPU: (total, d_rgb, d_opa) with the trainer's loss scale applied to the loss."""
    import torch.nn.functional as Fn
    r = torch.from_numpy(b["rgb"]).to(dtype).requires_grad_(True)
    o = torch.from_numpy(b["opa"]).to(dtype).requires_grad_(True)
    want = b["w_rgb"] * Fn.mse_loss(r, torch.from_numpy(b["pix"]).to(dtype)) + b["w_sky"] * Fn.binary_cross_entropy(o, 1 - torch.from_numpy(b["sky"]).to(dtype))
    (want * (b["up"] * b["grad_scale"])).backward()
    return float(want.detach()), r.grad.double().numpy(), o.grad.double().numpy()


# -------------------------------------------------------------------------------------------------------------- lidar
def lidar_masks(gt, t, eps, max_depth):
    """The integer facts, from the fp32 comparisons the reference performs: one correctly rounded fp32 subtraction / addition."""
    g = np.asarray(gt, F32).reshape(-1)
    t = np.asarray(t, F32)
    lo, hi = (g - F32(eps)).astype(F32), (g + F32(eps)).astype(F32)
    empty = t < lo[:, None]
    near = (t > lo[:, None]) & (t < hi[:, None])
    valid = (g > F32(0.01)) & (g < F32(max_depth))
    return dict(lo=lo, hi=hi, empty=empty, near=near, valid=valid, pos=g > 0)


def restate_lidar(depth, gt, w, t, eps, max_depth, w_depth, w_sight, up=1.0):
    """w_depth DepthLoss("l2") + w_sight compute_line_of_sight_loss in fp64.  ``total_ref`` is the reference's value: NaN when
    no ray is valid (the mean of an empty tensor); ``total`` / ``rays`` follow the kernel there: a depth term of 0."""
    m = lidar_masks(gt, t, eps, max_depth)
    dep, g, w64, t64 = (np.asarray(a, F64) for a in (np.asarray(depth).reshape(-1), np.asarray(gt).reshape(-1), w, t))
    R, S = w64.shape
    n_pos, n_valid = int(m["pos"].sum()), int(m["valid"].sum())
    # depth: mean over the valid rays of (clamp(pred / max) - clamp(gt / max))^2
    pn = dep / max_depth
    pn32 = (np.asarray(depth, F32).reshape(-1) / F32(max_depth)).astype(F32)
    passes = (pn32 >= 0) & (pn32 <= 1)                 # torch.clamp passes the gradient where min <= x <= max
    pc, gn = np.clip(pn, 0.0, 1.0), np.clip(g / max_depth, 0.0, 1.0)
    d = pc - gn
    depth_term = float((d[m["valid"]] ** 2).mean()) if n_valid else float("nan")
    ray_depth = np.where(m["valid"], w_depth * d * d / max(n_valid, 1), 0.0)
    d_depth = np.where(m["valid"] & passes, up * w_depth * 2.0 * d / (max_depth * max(n_valid, 1)), 0.0)
    # line of sight
    sigma = eps / 3
    x = t64 - g[:, None]
    arg = (x ** 2) / (2 * sigma ** 2)
    delta = (1 / (math.sqrt(2 * math.pi * sigma ** 2))) * np.exp(-arg)
    e = w64 - delta
    term = np.where(m["empty"], w64 ** 2, np.where(m["near"], e ** 2, 0.0))
    dterm = np.where(m["empty"], 2 * w64, np.where(m["near"], 2 * e, 0.0))
    empty_loss = (w64 ** 2 * m["empty"]).sum(1).mean()
    near_loss = (e ** 2 * m["near"]).sum(1).mean()
    sight = float(((empty_loss + near_loss) * m["pos"]).mean())      # scalar mean x per-ray mask, then the mean
    scale = w_sight * (n_pos / R) / R
    rays = ray_depth + scale * term.sum(1)
    total_ref = w_depth * depth_term + w_sight * sight
    st = dict(m, R=R, S=S, n_pos=n_pos, n_valid=n_valid, passes=passes, pc=pc, gn=gn, d=d, ray_depth=ray_depth, d_depth=d_depth, x=x, arg=arg,
              delta=delta, e=e, w=w64, term=term, scale=scale, up=float(up), w_depth=float(w_depth), w_sight=float(w_sight),
              max_depth=float(max_depth), sight=sight, rays=rays, total=float(rays.sum()), total_ref=total_ref,
              d_w=up * scale * dterm)
    if n_valid:
        assert abs(st["total"] - total_ref) <= 1e-12 * max(abs(total_ref), 1e-30) + 1e-300, "restatement: per-ray shares do not add up"
    return st


def _wave_rows(terms, dt):
    """Per-lane sequential sums over s = lane, lane + 64, ... then the xor butterfly; lane 0.  One row per ray."""
    R, S = terms.shape
    pad = (-S) % 64
    ch = np.concatenate([terms, np.zeros((R, pad), dt)], 1).reshape(R, -1, 64)
    part = np.zeros((R, 64), dt)
    for c in range(ch.shape[1]):
        part = part + ch[:, c]
    lanes = np.arange(64)
    off = 32
    while off:
        part = part + part[:, lanes ^ off]
        off >>= 1
    return part[:, 0]


def model_lidar(depth, gt, w, t, eps, max_depth, w_depth, w_sight, up=1.0, dt=F32, mut=""):
    """lidar_counts_kernel + lidar_loss_kernel (+ reduce_sum): per-ray loss shares, total, d_depth, d_weights."""
    cf = _cf(dt)
    g32, t32 = np.asarray(gt, F32).reshape(-1), np.asarray(t, F32)
    dep, g, wv, tv = np.asarray(depth, dt).reshape(-1), g32.astype(dt), np.asarray(w, dt), t32.astype(dt)
    R, S = wv.shape
    epsf, mx, wd, wsg, upf = cf(eps), cf(max_depth), cf(w_depth), cf(w_sight), dt(up)
    lo, hi = (g32 - F32(eps)).astype(F32)[:, None], (g32 + F32(eps)).astype(F32)[:, None]
    pos = g32 > 0
    valid = ((g32 >= F32(0.01)) if mut == "valid_ge" else (g32 > F32(0.01))) & ((g32 <= F32(max_depth)) if mut == "valid_le" else (g32 < F32(max_depth)))
    n_pos, n_valid = dt(pos.sum()), dt(valid.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        pn = dep / mx
        pn32 = (np.asarray(depth, F32).reshape(-1) / F32(max_depth)).astype(F32)
        gn, pc = np.clip(g / mx, dt(0), dt(1)), np.clip(pn, dt(0), dt(1))
        d = pc - gn
        nd = n_pos if mut == "mean_npos" else dt(R) if mut == "mean_R" else n_valid
        on = valid & (wd != 0)
        l = np.where(on, wd * d * d / nd, dt(0)).astype(dt)
        passes = ((pn32 > 0) & (pn32 < 1)) if mut == "clamp_strict" else np.ones(R, bool) if mut == "clamp_pass" else ((pn32 >= 0) & (pn32 <= 1))
        dd = np.where(on & passes, upf * wd * dt(2) * d / (mx * nd), dt(0)).astype(dt)
    if mut == "no_posfactor":
        scale = np.full(R, wsg / dt(R), dt)
    elif mut == "posfactor_per_ray":
        scale = (wsg * pos.astype(dt) / dt(R)).astype(dt)
    else:
        scale = np.full(R, wsg * (n_pos / dt(R)) / dt(R), dt)
    sigma = epsf if mut == "sigma_eps" else epsf / dt(3)
    pi = dt(PI32) if dt is F32 else F64(math.pi)
    if mut == "norm_pi":
        pi = dt(3.14159)
    norm = dt(1) / np.sqrt(dt(2) * pi * sigma * sigma)
    if mut == "norm_rsqrt":
        norm = np.nextafter(norm, dt(0))
    inv2s2 = dt(1) / (dt(2) * sigma * sigma)
    empty = (t32 <= lo) if mut == "le_empty" else (t32 < lo)
    near = ~empty & ((t32 >= lo) if mut == "le_near_lo" else (t32 > lo)) & ((t32 <= hi) if mut == "le_near_hi" else (t32 < hi))
    x = tv - g[:, None]
    e = wv - norm * np.exp(-(x * x) * inv2s2)
    term = np.where(empty, wv * wv, np.where(near, e * e, dt(0))).astype(dt)
    dw = np.where(empty, dt(2) * wv, np.where(near, dt(2) * e, dt(0))).astype(dt)
    if mut == "far":
        far = ~empty & ~near & (t32 > hi)
        term, dw = np.where(far, wv * wv, term).astype(dt), np.where(far, dt(2) * wv, dw).astype(dt)
    s_idx = np.arange(S)[None, :]
    if mut == "tail_lanes":
        term, dw = np.where(s_idx < (S // 64) * 64, term, dt(0)), np.where(s_idx < (S // 64) * 64, dw, dt(0))
    if mut == "first64":
        term, dw = np.where(s_idx < 64, term, dt(0)), np.where(s_idx < 64, dw, dt(0))
    acc = _wave_rows(term.astype(dt), dt)
    rays = (l + scale * acc).astype(dt)
    d_w = ((upf * scale)[:, None] * dw).astype(dt)
    if mut == "skip_nonpos":
        rays, dd, d_w = np.where(pos, rays, dt(0)), np.where(pos, dd, dt(0)), np.where(pos[:, None], d_w, dt(0))
    return dict(rays=rays.astype(dt), total=model_reduce(rays) if dt is F32 else F64(rays.sum()), d_depth=dd, d_w=d_w.astype(dt),
                n_pos=float(n_pos), n_valid=float(n_valid))


LIDAR_R = (1, 2, 3, 4, 5, 8, 13, 16)     # 2, 3 and 1 rays left in the last workgroup (R = 2, 3, 5 / 13); 8 and 16: every ray kind
LIDAR_S = (1, 2, 63, 64, 65, 128, 129, 200)
LIDAR_BATCHES = ("mixed", "novalid", "nopos", "allvalid", "w_depth0", "w_sight0")
MAXD = 64.0
STEP = 0.125
_THR = F32(0.01)
KINDS = {"zero": 0.0, "neg": -2.0, "thr": float(_THR), "thr_up": float(np.nextafter(_THR, F32(1))), "max": MAXD,
         "max_dn": float(np.nextafter(F32(MAXD), F32(0))), "normal": None}
_ALL = ("normal", "zero", "neg", "thr", "thr_up", "max", "max_dn")
_MIXED = {2: ("normal", "neg"), 4: ("normal", "neg", "thr_up", "zero"), 8: ("zero", "neg", "thr", "thr_up", "max", "normal", "zero", "neg"),
          16: _ALL + ("normal", "max", "thr") + ("neg", "zero") * 3}     # gt > 0 and valid counts are powers of two


def _kinds(R, batch, seed):
    if batch == "novalid":
        pool = ("zero", "neg", "thr", "max")
    elif batch == "nopos":
        pool = ("zero", "neg")
    elif batch == "allvalid":
        pool = ("normal", "thr_up", "max_dn", "normal")
    elif R in _MIXED:
        return list(_MIXED[R])
    else:
        pool = _ALL
        return [pool[(r + seed) % len(pool)] for r in range(R)]
    return [pool[r % len(pool)] for r in range(R)]


def build_lidar(R, S, batch="mixed", seed=0):
    """t on multiples of 2^-3 in [0, 70], weights k 2^-6, gt and eps dyadic (eps = 2.5 or 4), max_depth = 64, w_depth = 2^-1,
    w_sight = 2^-2, upstream 2^3.  Ray kinds: gt in {0, -2, 0.01f, its upper neighbour, max_depth, its lower neighbour, a
    multiple of 2^-3 in [8, 56]}; rendered depth / max cycles through {below 0, 0, 1, above 1, inside}.  Every ray gets the
    samples gt - eps, gt + eps, one grid step on either side of each, and gt itself (those that are >= 0), placed in the
    first lanes, at lanes 62..65, or in the last chunk; every other 'normal' ray has its near band emptied -- half of those but
    for one sample on gt -- so that its loss is exact.  The negative-gt ray keeps samples below gt + eps."""
    rng = np.random.default_rng(7919 * seed + 131 * R + S + 17 * LIDAR_BATCHES.index(batch))
    eps = 2.5 if seed % 2 else 4.0
    kinds = _kinds(R, batch, seed)
    gt = np.array([KINDS[k] if KINDS[k] is not None else rng.integers(64, 449) / 8.0 for k in kinds], F64).astype(F32)
    inside = rng.integers(1, 511, R) / 8.0
    depth = np.array([(-8.0, 0.0, MAXD, 72.0, inside[r])[(r + seed) % 5] for r in range(R)], F32)
    t = (rng.integers(0, 561, (R, S)) / 8.0).astype(F32)
    w = (rng.integers(0, 9, (R, S)) / 64.0).astype(F32)
    m = lidar_masks(gt, t, eps, MAXD)
    gap = np.zeros(R, bool)
    for r in range(R):
        lo, hi, g = float(m["lo"][r]), float(m["hi"][r]), float(gt[r])
        vals = [v for v in (lo - STEP, lo, lo + STEP, g, hi - STEP, hi, hi + STEP) if v >= 0.0]
        place = ("first", "mid", "last")[(r + seed) % 3]
        if S <= len(vals):
            pos = list(range(S))
            vals = [vals[(r + seed + s) % len(vals)] for s in range(S)]
        elif place == "mid" and S >= 66 and len(vals) == 7:
            pos, vals = [62, 63, 64, 65, 0, 1, 2], [vals[0], vals[1], vals[5], vals[6], vals[2], vals[4], vals[3]]
        elif place == "first":
            pos = list(range(len(vals)))
        else:
            pos = list(range(S - len(vals), S))
        t[r, pos] = np.array(vals, F32)
        if kinds[r] == "normal" and (r + seed) % 2 == 1 and S > 7:
            inb = (t[r] > m["lo"][r]) & (t[r] < m["hi"][r])
            at = np.flatnonzero(inb & (t[r] == gt[r]) & (np.arange(S) < 64))
            t[r, inb] = F32(lo - 1.0)
            if (r + seed) % 4 == 1:          # ... but for one sample on gt, in the first chunk: the only one in the band
                t[r, at[0] if at.size else 3] = gt[r]
            gap[r] = True
    b = dict(R=R, S=S, batch=batch, eps=eps, max_depth=MAXD, w_depth=0.0 if batch == "w_depth0" else 0.5,
             w_sight=0.0 if batch == "w_sight0" else 0.25, up=8.0, depth=depth, gt=gt, w=w, t=t, kinds=kinds, gap=gap)
    st = restate_lidar(depth, gt, w, t, eps, MAXD, b["w_depth"], b["w_sight"], b["up"])
    b["ref"] = st
    # preconditions: the thresholds of the grid rays are exact, the empty-band terms exact, their sums below 2^24 units
    grid_ray = np.array([k in ("normal", "zero", "neg", "max") for k in kinds])
    assert np.array_equal(st["lo"][grid_ray].astype(F64), gt[grid_ray].astype(F64) - eps), "lidar probe broken: gt - eps not exact"
    assert _exact32(w.astype(F64) ** 2) and float((w.astype(F64) ** 2).sum(1).max() * 2.0 ** 12) < BUDGET, "lidar probe broken: w^2 sums"
    if batch == "novalid":
        assert st["n_valid"] == 0 and math.isnan(st["total_ref"])
    if batch == "nopos":
        assert st["n_pos"] == 0
    if batch == "allvalid":
        assert st["n_valid"] == R
    b["stats"] = dict(on_lo=int((t == st["lo"][:, None]).sum()), on_hi=int((t == st["hi"][:, None]).sum()),
                      on_gt=int((t == gt[:, None]).sum()), near=int(st["near"].sum()), empty=int(st["empty"].sum()))
    return b


LIDAR_CASES = [(R, S, "mixed") for R in LIDAR_R for S in LIDAR_S] + [(R, S, bt) for bt in LIDAR_BATCHES[1:] for R, S in ((1, 65), (4, 64), (5, 200), (13, 2))]
LIDAR_REAL = [(R, S, eps, ws) for R, S in ((13, 65), (5, 200), (300, 128)) for eps in (6.0, 3.7, 2.5) for ws in (0.1, 0.1 * 2.0 ** -3)]


def lidar_norm32(eps):
    """norm of the Gaussian by the kernel's fp32 chain -- sigma = fl(fl(eps) / 3), 1 / sqrtf(((2 pi_f) sigma) sigma) -- every
    operation correctly rounded (the build has no fast-math flag)."""
    sigma = F32(eps) / F32(3)
    return F32(1) / np.sqrt(F32(2) * PI32 * sigma * sigma)


def lidar_exact_flags(b):
    """Which outputs of a lidar probe are exact, and their expected values (``want``: the restatement, with the entries below
    replaced).  The fp32 chain of `scale` equals its fp64 value where R and the gt > 0 count are powers of two; then

    * an empty-band gradient entry is an exact product;
    * a near-band sample ON gt has expf(-0) = 1, so delta is the fp32 `norm` itself -- taken from the fp32 chain, the way the
      masks are taken from the fp32 comparisons -- and d_w = fl32(w - norm32) 2 up scale bit for bit (norm 1 is exact: a
      contracted multiply-add changes nothing);
    * a ray's depth part is exact when d, w_depth d d / n_valid are representable;
    * a ray's loss is exact when no sample lies in its near band; where its only near-band samples sit on gt, each in the first
      64-sample chunk and alone in the band for its lane, the loss is the kernel's own fp32 sum: fl(e e) enters an empty lane
      (with or without contraction), every later addend w w is exact, the butterfly's order is fixed, and scale is a power of
      two."""
    st = b["ref"]
    R, S = st["R"], st["S"]
    sc32 = F32(F32(b["w_sight"]) * (F32(st["n_pos"]) / F32(R)) / F32(R))
    scale_ok = float(sc32) == st["scale"]
    nv = max(st["n_valid"], 1)
    d, wd = st["d"], st["w_depth"]
    dep_ok = _is_exact32(d) & _is_exact32(wd * d) & _is_exact32(wd * d * d) & _is_exact32(st["ray_depth"]) | ~st["valid"] | (wd == 0.0)
    dd_ok = dep_ok & _is_exact32(st["d_depth"]) & _is_exact32(st["max_depth"] * nv)
    on_gt = st["near"] & (st["x"] == 0.0)
    e32 = (np.asarray(b["w"], F32) - lidar_norm32(b["eps"])).astype(F32)
    want_dw = np.where(on_gt, st["up"] * st["scale"] * 2.0 * e32.astype(F64), st["d_w"])
    dw_ok = np.broadcast_to(scale_ok, st["d_w"].shape) & (~st["near"] | on_gt) & _is_exact32(want_dw)
    # the loss of a ray whose near band holds only samples on gt
    s_idx = np.arange(S)[None, :]
    lane_alone = np.ones(R, bool)
    for r in range(R):
        lanes = np.flatnonzero(on_gt[r]) % 64
        lane_alone[r] = np.unique(lanes).size == lanes.size
    only_gt = st["near"].any(1) & (st["near"] == on_gt).all(1) & ~(on_gt & (s_idx >= 64)).any(1) & lane_alone
    w32 = np.asarray(b["w"], F32)
    term32 = np.where(st["empty"], w32 * w32, np.where(on_gt, e32 * e32, F32(0))).astype(F32)
    acc32 = _wave_rows(term32, F32)
    want_rays = np.where(only_gt, (st["ray_depth"].astype(F32) + sc32 * acc32).astype(F64), st["rays"])
    sums = st["scale"] * st["term"].sum(1)
    ray_ok = dep_ok & scale_ok & (only_gt | ~st["near"].any(1) & _is_exact32(sums) & _is_exact32(st["rays"]))
    return dict(rays=ray_ok, d_depth=dd_ok, d_w=dw_ok, on_gt=on_gt, only_gt=only_gt, want=dict(rays=want_rays, d_depth=st["d_depth"], d_w=want_dw))


def check_lidar_outputs(b, rays, total, d_depth, d_w, what, exact=True, report=None):
    """Every per-ray loss and gradient entry inside its bound (tests/_bounds.lidar_bounds); on a probe (``exact``) the bound of
    every entry named by ``lidar_exact_flags`` is 0: it must equal the expected value as a number.  A sample outside both
    bands, an invalid ray's depth gradient and a blocked clamp have a bound of 0 in any case."""
    from tests._bounds import assert_err_bound, lidar_bounds
    st = b["ref"]
    bd = lidar_bounds(st, b["eps"])
    want = dict(rays=st["rays"], d_depth=st["d_depth"], d_w=st["d_w"])
    if exact:
        fl = lidar_exact_flags(b)
        bd = {k: np.where(fl[k], 0.0, v) for k, v in bd.items()}
        want = {k: np.where(fl[k], fl["want"][k], want[k]) for k in want}
    out = {}
    if rays is not None:
        out["rays"] = assert_err_bound(rays, want["rays"], bd["rays"], f"{what} per-ray loss", report)
    if d_depth is not None:
        out["d_depth"] = assert_err_bound(d_depth, want["d_depth"], bd["d_depth"], f"{what} d_depth", report)
    if d_w is not None:
        out["d_w"] = assert_err_bound(d_w, want["d_w"], bd["d_w"], f"{what} d_weights", report)
    if total is not None and rays is not None:
        want_t = F32(np.asarray(rays, F32).astype(F64).sum())
        assert F32(total) == want_t, f"{what}: total {float(total)!r} is not the double sum of the per-ray values rounded once ({float(want_t)!r})"
    return out


def realistic_lidar(R, S, eps, w_sight, seed=0):
    """Sorted midpoints in [0.1, 90], weights from a thin wall near gt plus rand^2 1e-3 elsewhere, gt in [-5, 95]."""
    g = torch.Generator().manual_seed(31 * seed + 7 * R + S)
    t = torch.sort(torch.rand(R, S, generator=g) * 89.9 + 0.1, -1).values
    gt = torch.rand(R, generator=g) * 100 - 5
    wall = 0.5 * torch.exp(-0.5 * ((t - (gt[:, None] + 0.3 * torch.randn(R, 1, generator=g))) / 0.4) ** 2)
    w = wall + torch.rand(R, S, generator=g) ** 2 * 1e-3
    depth = torch.rand(R, generator=g) * 100 - 5
    b = dict(R=R, S=S, eps=float(eps), max_depth=80.0, w_depth=1.0, w_sight=float(w_sight), up=1024.0, depth=depth.numpy(), gt=gt.numpy(),
             w=w.numpy(), t=t.numpy())
    b["ref"] = restate_lidar(b["depth"], b["gt"], b["w"], b["t"], b["eps"], 80.0, 1.0, b["w_sight"], b["up"])
    return b


def ref_lidar_torch(b, dtype=torch.float32):
    """The reference's lines evaluated by torch on the CPU in ``dtype`` (masks from the fp32 tensors, as the reference forms
    them): per-ray shares are not available there -- (total, d_depth, d_w)."""
    eps, mx = b["eps"], b["max_depth"]
    g32, t32 = torch.from_numpy(b["gt"]), torch.from_numpy(b["t"])
    dep = torch.from_numpy(b["depth"]).to(dtype).requires_grad_(True)
    w = torch.from_numpy(b["w"]).to(dtype).requires_grad_(True)
    g, t = g32.to(dtype), t32.to(dtype)
    valid = (g32 > 0.01) & (g32 < mx)
    norm = lambda v: torch.clamp(v / mx, 0.0, 1.0)  # noqa: E731
    depth_loss = ((norm(dep[valid]) - norm(g[valid])) ** 2).mean()
    gd32 = g32.unsqueeze(-1)
    empty = t32 < gd32 - eps
    near = (t32 > (gd32 - eps)) & (t32 < gd32 + eps)
    sigma = eps / 3
    delta = (1 / (math.sqrt(2 * torch.pi * sigma ** 2))) * torch.exp(-((t - g.unsqueeze(-1)) ** 2) / (2 * sigma ** 2))
    empty_loss = (w.square() * empty).sum(-1, keepdim=True).mean()
    near_loss = ((w - delta).square() * near).sum(-1, keepdim=True).mean()
    sight = ((empty_loss + near_loss) * (g32 > 0)).mean()
    want = b["w_depth"] * depth_loss + b["w_sight"] * sight
    (want * b["up"]).backward()
    return float(want.detach()), dep.grad.double().numpy(), w.grad.double().numpy()


# ---------------------------------------------------------------------------------------------------------------- reg
REG_THREADS, REG_MAX_BLOCKS = 256, 1024


def reg_blocks(n_max):
    return int(min(max(-(-int(n_max) // (REG_THREADS * 4)), 1), REG_MAX_BLOCKS))


def _cycle_operands(T, mut=""):
    """(ff, fpb, bf, bpf) as flat [n_flow] arrays, from the four slices or from the packed pair flow6 [N, 6], flow2 [2 N, 6]."""
    if "flow2" in T:
        f6, f2 = T["flow6"].reshape(-1, 6), T["flow2"].reshape(-1, 6)
        N = f6.shape[0]
        fpb = f2[:N, :3] if mut == "swap_blocks" else f2[:N, 3:]
        bpf = (f2[N:, 3:] if mut == "swap_blocks" else f2[:N, :3] if mut == "second_half" else f2[N:, :3])
        return f6[:, :3].reshape(-1), fpb.reshape(-1), f6[:, 3:].reshape(-1), bpf.reshape(-1)
    if "fpb" in T:
        return tuple(T[k].reshape(-1) for k in ("ff", "fpb", "bf", "bpf"))
    return None


def _reg_terms(T, coefs, dt, mut=""):
    """[(name, per-element term, c, n)] in the kernel's order."""
    out = []
    for name in ("dyn", "shadow"):
        if name in T:
            x = np.asarray(T[name], dt).reshape(-1)
            out.append((name, x, coefs[name], x.size))
    if "feat" in T:
        d = np.asarray(T["feat"], dt).reshape(-1) - np.asarray(T["feat_gt"], dt).reshape(-1)
        out.append(("feat", d * d, coefs["feat"], d.size))
    cyc = _cycle_operands(T, mut)
    if cyc is not None:
        ff, fpb, bf, bpf = (np.asarray(a, dt) for a in cyc)
        u, v = ff + fpb, bf + bpf
        out.append(("cycle", u * u if mut == "cycle_second" else u * u + v * v, coefs["cycle"], u.size))
    return out


def restate_reg(T, coefs, base=None, up=1.0, grad_scale=1.0):
    """base + c_dyn mean(dyn) + c_shadow mean(shadow) + c_feat mean((feat - gt)^2) + c_cycle mean((ff + fpb)^2 + (bf + bpf)^2) in
    fp64 and the gradients (base's: the upstream, unscaled; the regularisers': times grad_scale; none to ff / bf)."""
    terms = _reg_terms(T, coefs, F64)
    k = float(up) * float(grad_scale)
    total = float(base) if base is not None else 0.0
    st = dict(grads={}, d_base=float(up) if base is not None else None, parts={})
    for name, x, c, n in terms:
        st["parts"][name] = c * float(x.mean())
        total += st["parts"][name]
        if name in ("dyn", "shadow"):
            st["grads"][name] = np.full(T[name].shape, k * c / n)
    if "feat" in T:
        n = T["feat"].size
        st["grads"]["feat"] = k * 2.0 * coefs["feat"] / n * (np.asarray(T["feat"], F64) - np.asarray(T["feat_gt"], F64))
    cyc = _cycle_operands(T)
    if cyc is not None:
        ff, fpb, bf, bpf = (np.asarray(a, F64) for a in cyc)
        gk = k * 2.0 * coefs["cycle"] / ff.size
        if "flow2" in T:
            N = T["flow6"].reshape(-1, 6).shape[0]
            g2 = np.zeros((2 * N, 6))
            g2[:N, 3:], g2[N:, :3] = (gk * (ff + fpb)).reshape(N, 3), (gk * (bf + bpf)).reshape(N, 3)
            st["grads"]["flow2"] = g2
        else:
            st["grads"]["fpb"], st["grads"]["bpf"] = (gk * (ff + fpb)).reshape(T["fpb"].shape), (gk * (bf + bpf)).reshape(T["bpf"].shape)
    st["total"] = total
    return st


def _strided(x, stride, dt):
    pad = (-x.size) % stride
    rows = np.concatenate([x, np.zeros(pad, dt)]).reshape(-1, stride)
    s = np.zeros(stride, dt)
    for row in rows:
        s = s + row
    return s


def reg_geometry(T):
    """(blocks, stride) of the forward / backward launch: 1024 elements per block over the largest present count (the packed
    cycle term counts 4 n_flow = 12 N, the size of its gradient), at most 1024 blocks."""
    n = 1
    for name in ("dyn", "shadow", "feat"):
        if name in T:
            n = max(n, T[name].size)
    if "flow2" in T:
        n = max(n, T["flow2"].size)                           # 12 N
    elif "fpb" in T:
        n = max(n, T["fpb"].size)
    blocks = reg_blocks(n)
    return blocks, blocks * REG_THREADS


def model_reg(T, coefs, base=None, up=1.0, grad_scale=1.0, dt=F32, mut=""):
    """reg_losses_fwd_kernel + reg_losses_finish_kernel + reg_losses_bwd_kernel: block partials, total, gradients."""
    cf = _cf(dt)
    blocks, stride = reg_geometry(T)
    terms = _reg_terms(T, coefs, dt, mut)
    n_other = max(n for _, _, _, n in terms)
    l = np.zeros(stride, dt)
    for name, x, c, n in terms:
        if mut == "one_sweep":
            x = x[:stride]
        if mut == "tail" and x.size >= stride:
            x = x[:(x.size // stride) * stride]
        div = dt(n_other if mut == "divisor" else n)
        l = l + cf(c) / div * _strided(x.astype(dt), stride, dt)
    part = l.reshape(-1, 64)
    lanes = np.arange(64)
    off = 32
    while off:
        part = part + part[:, lanes ^ off]
        off >>= 1
    wp = part[:, 0].reshape(blocks, 4)
    partials = np.zeros(blocks, dt)
    for k in range(4):
        partials = partials + wp[:, k]
    # finish: 256 strided double sums, the butterfly in each of the four waves, (p0 + p1) + (p2 + p3), + base, one rounding
    p64 = partials.astype(F64)
    acc = _strided(p64, 256, F64).reshape(4, 64)
    off = 32
    while off:
        acc = acc + acc[:, lanes ^ off]
        off >>= 1
    tot = (float(base) if base is not None else 0.0) + ((acc[0, 0] + acc[1, 0]) + (acc[2, 0] + acc[3, 0]))
    out = dict(partials=partials, total=F32(tot) if dt is F32 else F64(tot), grads={}, d_ff=None,
               d_base=None if base is None else float(up) * (float(grad_scale) if mut == "base_scaled" else 1.0))
    upg = dt(up) * cf(grad_scale)
    for name in ("dyn", "shadow"):
        if name in T:
            out["grads"][name] = np.full(T[name].shape, upg * (cf(coefs[name]) / dt(T[name].size)), dt)
    if "feat" in T:
        gk = upg * (dt(2) * cf(coefs["feat"]) / dt(T["feat"].size))
        out["grads"]["feat"] = gk * (np.asarray(T["feat"], dt) - np.asarray(T["feat_gt"], dt))
    cyc = _cycle_operands(T, mut)
    if cyc is not None:
        ff, fpb, bf, bpf = (np.asarray(a, dt) for a in cyc)
        gk = upg * (dt(2) * cf(coefs["cycle"]) / dt(ff.size))
        if "flow2" in T:
            f6, f2 = np.asarray(T["flow6"], dt).reshape(-1, 6), np.asarray(T["flow2"], dt).reshape(-1, 6)
            N = f6.shape[0]
            g2 = (gk * (f2 + dt(1))).astype(dt) if mut == "unread_nonzero" else np.zeros((2 * N, 6), dt)   # (what the buffer held)
            g2[:N, 3:], g2[N:, :3] = (gk * (ff + fpb)).reshape(N, 3), (gk * (bf + bpf)).reshape(N, 3)
            out["grads"]["flow2"] = g2.astype(dt)
        else:
            out["grads"]["fpb"], out["grads"]["bpf"] = (gk * (ff + fpb)).reshape(T["fpb"].shape), (gk * (bf + bpf)).reshape(T["bpf"].shape)
        if mut == "grad_detached":
            out["d_ff"] = (gk * (ff + fpb))
    return out


REG_COUNTS = (1, 3, 255, 256, 257, 1023, 1024, 1025, 4097, 1048576, 1048577, 2097157)   # the last three: a thread owns more than four elements
REG_PACKED_ROWS = (1, 85, 86, 87382)                                                      # 12 N crosses 1024 and 1 048 576
REG_PATTERNS = ("d", "ds", "dsf", "dsfc", "c")                                            # what the trainer produces (with a base)
REG_K = dict(dyn=6, shadow=5, feat=4, cycle=7)


REG_REAL = [dict(R=64, S=16, E=8), dict(R=333, S=7, E=5), dict(R=9, S=1, E=1), dict(R=86, S=1, E=1, packed=True, terms="c"),
            dict(R=64, S=16, E=8, packed=True)]


def reg_families(big=True):
    """name -> builder arguments: single-term counts, the trainer's presence patterns, no base, the packed rows."""
    fam = {f"single {n}": dict(pattern="d", R=n) for n in REG_COUNTS if big or n < 100000}
    fam.update({f"pattern {p}": dict(pattern=p, R=37, S=5, E=3) for p in REG_PATTERNS})
    fam["nobase dsfc"] = dict(pattern="dsfc", R=37, S=5, E=3, with_base=False)
    fam.update({f"packed {N}": dict(pattern="c", R=N, packed=True) for N in REG_PACKED_ROWS if big or N < 1000})
    fam["packed dsfc"] = dict(pattern="dsfc", R=37, S=5, E=3, packed=True)
    return fam


def build_reg(pattern, R, S=1, E=1, packed=False, seed=0, with_base=True):
    """dyn [R, S] and shadow [R, 1] on k / 8 (k < 8), feat / feat_gt [R, E] on multiples of 1/4 in [0, 1], the flows [R, S, 3] on
    multiples of 1/4 in [-1/2, 1/2]; coefficient of a term = n 2^-k, so c / (float) n is exact; base 3.25, upstream 2^-1,
    grad_scale 2^4.  ``packed``: flow6 [N, 6] and flow2 [2 N, 6] are drawn whole -- the column blocks the loss must not read
    hold values of their own -- and the sliced form is cut from them, so both forms see the same numbers."""
    rng = np.random.default_rng(104729 * seed + 31 * R + 7 * S + E + 3 * len(pattern))
    T, coefs = {}, {}
    if "d" in pattern:
        T["dyn"] = (rng.integers(0, 8, (R, S)) / 8.0).astype(F32)
    if "s" in pattern:
        T["shadow"] = (rng.integers(0, 8, (R, 1)) / 8.0).astype(F32)
    if "f" in pattern:
        T["feat"], T["feat_gt"] = ((rng.integers(0, 5, (R, E)) / 4.0).astype(F32) for _ in range(2))
    if "c" in pattern:
        N = R * S
        f6, f2 = (rng.integers(-2, 3, (N, 6)) / 4.0).astype(F32), (rng.integers(-2, 3, (2 * N, 6)) / 4.0).astype(F32)
        if packed:
            T["flow6"], T["flow2"] = f6, f2
        else:
            T.update(ff=f6[:, :3].copy(), bf=f6[:, 3:].copy(), fpb=f2[:N, 3:].copy(), bpf=f2[N:, :3].copy())
    n_of = dict(dyn=R * S, shadow=R, feat=R * E, cycle=3 * R * S)
    for name, key in (("dyn", "d"), ("shadow", "s"), ("feat", "f"), ("cycle", "c")):
        coefs[name] = n_of[name] * 2.0 ** -REG_K[name] if key in pattern else 0.0
    b = dict(T=T, coefs=coefs, base=3.25 if with_base else None, up=0.5, grad_scale=16.0, pattern=pattern, packed=packed)
    st = restate_reg(T, coefs, b["base"], b["up"], b["grad_scale"])
    units, q = 0.0, 2
    for name, x, c, n in _reg_terms(T, coefs, F64):
        assert _exact32(c) and n < BUDGET and _exact32(x), f"reg probe broken: {name}"
        units += float(np.abs(x).sum()) * 2.0 ** -REG_K[name]
        q = max(q, REG_K[name] + grid_of(x))               # the finest grid a contribution (c / n) term lies on
    assert (units + abs(b["base"] or 0.0)) * 2.0 ** q < BUDGET, "reg probe broken: the sums are not exact in any order"
    assert _exact32(st["total"]) and all(_exact32(g) for g in st["grads"].values()), "reg probe broken: outputs not exact"
    b["ref"] = st
    return b


def check_reg_outputs(b, partials, total, grads, what, d_ff=None, d_base="skip"):
    """Exact: the total and every gradient entry equal the restatement; the total is also the double sum of the launch's own
    block partials plus base, rounded once; the detached flows get no gradient."""
    st = b["ref"]
    assert float(total) == st["total"], f"{what}: total {float(total)!r} vs {st['total']!r}"
    if partials is not None:
        assert not np.isnan(np.asarray(partials)).any(), f"{what}: a block partial was not written"
        assert float(F32(np.asarray(partials, F64).sum() + (b["base"] or 0.0))) == float(total), f"{what}: total is not the sum of the partials"
    for name, g in grads.items():
        if g is None:
            continue
        assert np.array_equal(np.asarray(g, F64).reshape(st["grads"][name].shape), st["grads"][name]), f"{what}: gradient of {name} differs"
    assert d_ff is None, f"{what}: the detached flows received a gradient"
    if d_base != "skip":
        assert d_base == st["d_base"], f"{what}: base's gradient {d_base!r} vs {st['d_base']!r}"


def realistic_reg(R, S, E, seed=0, packed=False, terms="dsfc"):
    """The distributions of test_reg_losses_match_the_reference_expressions, the shipped coefficients, grad_scale 1024."""
    g = torch.Generator().manual_seed(R * 7 + S + seed)
    base = float(torch.rand((), generator=g))
    T = {}
    dyn, sh = torch.rand(R, S, generator=g) * 3, torch.rand(R, 1, generator=g)
    ft, gt = torch.randn(R, E, generator=g), torch.rand(R, E, generator=g)
    N = R * S
    f6, f2 = torch.randn(N, 6, generator=g) * 0.3, torch.randn(2 * N, 6, generator=g) * 0.3
    if "d" in terms:
        T["dyn"] = dyn.numpy()
    if "s" in terms:
        T["shadow"] = sh.numpy()
    if "f" in terms:
        T["feat"], T["feat_gt"] = ft.numpy(), gt.numpy()
    if "c" in terms:
        if packed:
            T["flow6"], T["flow2"] = f6.numpy(), f2.numpy()
        else:
            T.update(ff=f6[:, :3].contiguous().numpy(), bf=f6[:, 3:].contiguous().numpy(), fpb=f2[:N, 3:].contiguous().numpy(),
                     bpf=f2[N:, :3].contiguous().numpy())
    coefs = dict(dyn=0.01, shadow=0.01, feat=0.5, cycle=0.005)
    b = dict(T=T, coefs=coefs, base=float(F32(base)), up=1.0, grad_scale=1024.0, packed=packed)
    b["ref"] = restate_reg(T, coefs, b["base"], 1.0, 1024.0)
    return b


def reg_block_refs(b):
    """fp64 value and abs-sum bound of every block partial of the launch (tests/_bounds.reg_partial_bound)."""
    from tests._bounds import reg_partial_bound
    blocks, stride = reg_geometry(b["T"])
    ref, err = np.zeros(blocks), np.zeros(blocks)
    for name, x, c, n in _reg_terms(b["T"], b["coefs"], F64):
        blk = (np.arange(n) % stride) // REG_THREADS
        s = np.bincount(blk, weights=x, minlength=blocks)
        a = np.bincount(blk, weights=np.abs(x), minlength=blocks)
        ref += c / n * s
        err += reg_partial_bound(name, n, stride) * U * abs(c) / n * a
    return ref, err


def check_reg_realistic(b, partials, total, grads, what, report=None):
    """Every block partial inside its abs-sum bound, the total the double sum of the launch's own partials plus base rounded
    once, every gradient entry within its few roundings of the fp64 restatement, exact zeros in the unread packed blocks."""
    from tests._bounds import C_REG_GRAD, C_REG_GRAD_CONST, assert_err_bound
    st = b["ref"]
    out = {}
    if partials is not None:
        ref, err = reg_block_refs(b)
        out["partials"] = assert_err_bound(partials, ref, err, f"{what} block partials", report)
        assert float(F32(np.asarray(partials, F32).astype(F64).sum() + (b["base"] or 0.0))) == float(total), f"{what}: total is not the sum of the partials"
        lim = float(err.sum()) + U * abs(st["total"])
        assert abs(float(total) - st["total"]) <= lim, f"{what}: total {float(total)!r} vs fp64 {st['total']!r}, bound {lim:.3e}"
    for name, g in grads.items():
        if g is None:
            continue
        r = st["grads"][name]
        c = C_REG_GRAD_CONST if name in ("dyn", "shadow") else C_REG_GRAD
        a = np.abs(r)      # (fl(a - b) and fl(a + b) of fp32 inputs carry a RELATIVE u; an unread packed entry is exactly 0)
        out[name] = assert_err_bound(g, r, c * U * a, f"{what} d_{name}", report)
    return out


def ref_reg_torch(b, dtype=torch.float32):
    """The reference's expressions by torch on the CPU in ``dtype``: (total, {name: gradient})."""
    T, c = b["T"], b["coefs"]
    lv = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).requires_grad_(k not in ("feat_gt", "ff", "bf", "flow6")) for k, v in T.items()}
    reg = torch.zeros((), dtype=dtype)
    if "dyn" in lv:
        reg = reg + c["dyn"] * lv["dyn"].mean()
    if "shadow" in lv:
        reg = reg + c["shadow"] * lv["shadow"].mean()
    if "feat" in lv:
        reg = reg + c["feat"] * torch.nn.functional.mse_loss(lv["feat"], lv["feat_gt"])
    if "flow2" in lv:
        N = lv["flow6"].shape[0]
        reg = reg + c["cycle"] * ((lv["flow6"][:, :3] + lv["flow2"][:N, 3:]) ** 2 + (lv["flow6"][:, 3:] + lv["flow2"][N:, :3]) ** 2).mean()
    elif "fpb" in lv:
        reg = reg + c["cycle"] * ((lv["ff"].detach() + lv["fpb"]) ** 2 + (lv["bf"].detach() + lv["bpf"]) ** 2).mean()
    total = reg + (b["base"] or 0.0)
    (reg * (b["up"] * b["grad_scale"])).backward()
    return float(total.detach()), {k: v.grad.double().numpy() for k, v in lv.items() if v.grad is not None}
