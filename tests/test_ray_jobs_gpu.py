"""emer_ray_jobs (csrc/rayinputs.hip): the per-ray stages of the colour heads as members of one launch, against the stand-alone
entry points -- the trusted side, held bit for bit to fp64 by test_ray_exact_gpu.py and per entry by test_kernels_gpu.py.  A member must compute what its
own launch computes BIT FOR BIT (same stage function, same per-lane work); the exceptions are the two stages that leave with
relaxed float atomics from more than one workgroup per target, where neither side is reproducible:

  * ray_wgrad beyond one 256-row chunk: both sides against an fp64 product with test_ray_wgrad_matches_fp64's bound;
  * the reduction of a fused backward's partials once the partial blocks are cut into more than one range (>= 16 blocks): both
    sides against the fp64 sum of the very partials, per entry |err| <= (n_blocks + 1) 2^-24 sum|partial| (+ the target's ulp).

Row counts: 1 and 33 (below / above the 32-row tile), 257 (one row past ray_wgrad's chunk), 600 (two chunks and a partial
128-row round).  Widths of the shipped static config: Kh = 33 (direction PE, max_deg 4) + 16 (embedding), hidden 64, 3 outputs.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = [1, 33, 257, 600]
MAX_DEG, E, H, C = 4, 16, 64, 3
P = 3 * (1 + 2 * (MAX_DEG + 1))
KH = P + E


def _dev():
    return torch.device("cuda:0")


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(_dev())


def _case(R, n_emb, seed=0):
    """Inputs and parameters of both heads; indices leave the table's last row unused."""
    g = torch.Generator().manual_seed(1000 * R + 10 * n_emb + seed)
    d = torch.randn(R, 3, generator=g)
    c = dict(R=R, n_emb=n_emb)
    c["dirs"] = (d / d.norm(dim=1, keepdim=True)).to(_dev())
    c["idx"] = torch.randint(0, n_emb - 1, (R,), generator=g).to(_dev())
    c["emb"] = _rand(g, n_emb, E)
    # rgb head: [hray | geo] -> 64 -> (skip) -> 64 -> 3; only its per-ray column blocks matter here
    c["rgb"] = (_rand(g, H, KH + 64, scale=0.2), _rand(g, H), _rand(g, H, H + KH + 64, scale=0.2), _rand(g, H))
    c["sky"] = (_rand(g, H, KH, scale=0.2), _rand(g, H), _rand(g, H, H + KH, scale=0.2), _rand(g, H), _rand(g, C, H, scale=0.2), _rand(g, C))
    c["g"] = g
    return c


def _forward_standalone(c):
    """emer_ray_inputs_fwd -> emer_ray_pre_fwd (twice) -> emer_ray_head_fwd."""
    from emernerf_amd import _lib
    from emernerf_amd._lib import ACT_SIGMOID
    R, dev = c["R"], _dev()
    o = dict(out_rgb=torch.empty(R, KH, device=dev), out_sky=torch.empty(R, KH, device=dev), rb_rgb=torch.empty(R, 2 * H, device=dev),
             rb_sky=torch.empty(R, 2 * H, device=dev), a1=torch.empty(R, H, device=dev), a2=torch.empty(R, H, device=dev), out=torch.empty(R, C, device=dev))
    _lib.call("emer_ray_inputs_fwd", c["dirs"].data_ptr(), 3, c["idx"].data_ptr(), 1, c["emb"].data_ptr(), c["n_emb"], E, MAX_DEG, R,
              o["out_rgb"].data_ptr(), KH, o["out_sky"].data_ptr(), KH, _st())
    for x, (W0, B0, W1, B1), rb in ((o["out_rgb"], c["rgb"], o["rb_rgb"]), (o["out_sky"], c["sky"][:4], o["rb_sky"])):
        _lib.call("emer_ray_pre_fwd", x.data_ptr(), KH, R, KH, H, W0.data_ptr(), W0.stride(0), B0.data_ptr(), W1[:, H:].data_ptr(), W1.stride(0),
                  B1.data_ptr(), rb.data_ptr(), 2 * H, _st())
    W1, W2, B2 = c["sky"][2], c["sky"][4], c["sky"][5]
    _lib.call("emer_ray_head_fwd", o["rb_sky"].data_ptr(), 2 * H, R, W1.data_ptr(), W1.stride(0), W2.data_ptr(), B2.data_ptr(), C, ACT_SIGMOID,
              o["a1"].data_ptr(), o["a2"].data_ptr(), o["out"].data_ptr(), _st())
    return o


_CACHE = {}


def _shared(R, n_emb=3):
    """The case and its stand-alone forward, computed once and shared (read-only) among the tests."""
    key = (R, n_emb)
    if key not in _CACHE:
        c = _case(R, n_emb)
        _CACHE[key] = (c, _forward_standalone(c))
    return _CACHE[key]


@pytest.mark.parametrize("n_emb", [3, 7])
@pytest.mark.parametrize("R", ROWS)
def test_front_launch_equals_the_four_launches(hip_lib, R, n_emb):
    """The rgb chain inputs -> pre_fwd and the sky chain inputs -> pre_fwd -> head_fwd in one launch: every tensor a later launch or
    the backward reads is written, and written bit for bit as by the separate launches."""
    from emernerf_amd import ray_jobs as rj
    from emernerf_amd._lib import ACT_SIGMOID
    c, want = _shared(R, n_emb)
    dev = _dev()
    got = {k: torch.full_like(v, float("nan")) for k, v in want.items()}
    W0, B0, W1, B1, W2, B2 = c["sky"]
    RW0, RB0, RW1, RB1 = c["rgb"]
    jobs = [rj.fwd_chain_job(rj.inputs_args(c["dirs"], c["idx"], c["emb"], MAX_DEG, None, got["out_sky"]), rj.pre_fwd_args(got["out_sky"], W0, B0, W1, B1, got["rb_sky"]),
                             rj.head_fwd_args(got["rb_sky"], W1, W2, B2, ACT_SIGMOID, got["a1"], got["a2"], got["out"])),
            rj.fwd_chain_job(rj.inputs_args(c["dirs"], c["idx"], c["emb"], MAX_DEG, got["out_rgb"], None), rj.pre_fwd_args(got["out_rgb"], RW0, RB0, RW1, RB1, got["rb_rgb"]))]
    rj.launch(jobs, c["dirs"])
    torch.cuda.synchronize(dev)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def _sky_backward_standalone(c, fwd, dout):
    from emernerf_amd import _lib
    from emernerf_amd._lib import ACT_SIGMOID
    R, dev = c["R"], _dev()
    W0, _, W1, _, W2, _ = c["sky"]
    o = dict(dpre2=torch.empty(R, C, device=dev), dpre1=torch.empty(R, H, device=dev), dpre0=torch.empty(R, H, device=dev), dx=torch.empty(R, KH, device=dev))
    _lib.call("emer_ray_head_bwd", dout.data_ptr(), fwd["out"].data_ptr(), fwd["a1"].data_ptr(), fwd["a2"].data_ptr(), R, W1.data_ptr(), W1.stride(0),
              W2.data_ptr(), C, ACT_SIGMOID, o["dpre2"].data_ptr(), o["dpre1"].data_ptr(), o["dpre0"].data_ptr(), _st())
    _lib.call("emer_ray_pre_bwd", o["dpre0"].data_ptr(), o["dpre1"].data_ptr(), H, R, KH, H, W0.data_ptr(), W0.stride(0), W1[:, H:].data_ptr(), W1.stride(0),
              o["dx"].data_ptr(), KH, _st())
    return o


def _rgb_bwd_fused(c, R, S, t, ws, targets):
    """emer_rgb_head_bwd_fused on the tensors of `t` (its reduction is launched, or captured by the caller)."""
    from emernerf_amd import _lib
    RW0, _, RW1, _ = c["rgb"]
    tw0, tw1, tw2, tb2 = targets
    _lib.call("emer_rgb_head_bwd_fused", t["dout"].data_ptr(), t["out"].data_ptr(), t["a1"].data_ptr(), t["a2"].data_ptr(), t["geo"].data_ptr(), 64, R, S, KH,
              RW0.data_ptr(), RW1.data_ptr(), t["W2"].data_ptr(), t["dgeo"].data_ptr(), t["s1"].data_ptr(), t["s0"].data_ptr(), ws.data_ptr(),
              tw0.data_ptr(), tw0.stride(0), tw1.data_ptr(), tw1.stride(0), tw2.data_ptr(), tw2.stride(0), tb2.data_ptr(), _st())


def _reduce_reference(cap, ws, targets0):
    """fp64 sums of the captured reduction's partials on top of the targets' initial values, and the per-entry sums of |partial|."""
    nb, stride = cap.n_blocks, cap.stride
    part = ws[:nb * stride].view(nb, stride).double()
    want, mag = {}, {}
    for j in range(cap.n_jobs):
        q = cap.job[j]
        for ptr, n_el, name in ((q.dw, q.n * q.k, "w"), (q.db, q.n, "b")):
            if not ptr:
                continue
            t0 = targets0[ptr]
            if ptr not in want:
                want[ptr], mag[ptr] = t0.double().clone(), torch.zeros_like(t0, dtype=torch.float64)
            off = q.off + (0 if name == "w" else q.n * q.k)
            blk = part[:, off:off + n_el]
            s, a = blk.sum(0), blk.abs().sum(0)
            if name == "b":
                want[ptr] += s
                mag[ptr] += a
                continue
            s, a = s.view(q.n, q.k), a.view(q.n, q.k)
            segs = [(0, q.k, 0)] if q.n_segs == 0 else [(q.col[i], q.width[i], q.dst[i]) for i in range(q.n_segs)]
            for col, width, dst in segs:
                want[ptr][:, dst:dst + width] += s[:, col:col + width]
                mag[ptr][:, dst:dst + width] += a[:, col:col + width]
    return want, mag


@pytest.mark.parametrize("R", ROWS)
def test_launch_a_equals_the_chain_the_pre_bwd_and_the_reduction(hip_lib, R):
    """First level of the tail in one launch: the sky chain head_bwd -> pre_bwd, the rgb head's pre_bwd, the reduction of the rgb
    backward's partials (captured from emer_rgb_head_bwd_fused instead of launched by it)."""
    from emernerf_amd import _lib, ray_jobs as rj
    from emernerf_amd._lib import ACT_SIGMOID
    c, fwd = _shared(R)
    dev, S = _dev(), 16
    g = torch.Generator().manual_seed(R)
    dout = _rand(g, R, C)
    want = _sky_backward_standalone(c, fwd, dout)
    # the rgb backward, twice on the same operands: reduction launched by the entry point / captured and run as a job
    N = R * S
    t = dict(dout=_rand(g, N, C), out=torch.rand(N, C, generator=g).to(dev), a1=_rand(g, N, H).relu(), a2=_rand(g, N, H).relu(), geo=_rand(g, N, 64),
             W2=_rand(g, C, H, scale=0.2))
    RW0, _, RW1, _ = c["rgb"]
    n_ws = int(_lib.load().emer_rgb_head_bwd_fused_workspace(R, S))
    assert n_ws > 0
    init = [_rand(g, H, KH + 64), _rand(g, H, H + KH + 64), _rand(g, C, H), _rand(g, C)]   # targets that already hold a value

    def run(capture):
        tt = dict(t, dgeo=torch.empty(N, 64, device=dev), s1=torch.empty(R, H, device=dev), s0=torch.empty(R, H, device=dev))
        ws = torch.empty(n_ws, device=dev)
        targets = [x.clone() for x in init]
        cap = rj.DwReduceArgs()
        if capture:
            with rj.capture_dw_reduce(cap):
                _rgb_bwd_fused(c, R, S, tt, ws, targets)
            assert cap.n_jobs == 3 and cap.partials == ws.data_ptr()
        else:
            _rgb_bwd_fused(c, R, S, tt, ws, targets)
        return tt, ws, targets, cap

    t1, _, tgt1, _ = run(False)
    dh1 = torch.empty(R, KH, device=dev)
    _lib.call("emer_ray_pre_bwd", t1["s0"].data_ptr(), t1["s1"].data_ptr(), H, R, KH, H, RW0.data_ptr(), RW0.stride(0), RW1[:, H:].data_ptr(), RW1.stride(0),
              dh1.data_ptr(), KH, _st())
    t2, ws2, tgt2, cap = run(True)
    torch.cuda.synchronize(dev)
    assert all(torch.equal(a, b) for a, b in zip(tgt2, init)), "a captured reduction must not have run"
    assert torch.equal(t1["s0"], t2["s0"]) and torch.equal(t1["s1"], t2["s1"]) and torch.equal(t1["dgeo"], t2["dgeo"])
    W0, _, W1, _, W2, _ = c["sky"]
    got = {k: torch.full_like(v, float("nan")) for k, v in want.items()}
    dh2 = torch.full_like(dh1, float("nan"))
    rj.launch([rj.job(rj.DW_REDUCE, cap),
               rj.bwd_chain_job(rj.head_bwd_args(dout, fwd["out"], fwd["a1"], fwd["a2"], W1, W2, ACT_SIGMOID, got["dpre2"], got["dpre1"], got["dpre0"]),
                                rj.pre_bwd_args(got["dpre0"], got["dpre1"], KH, W0, W1, got["dx"])),
               rj.job(rj.PRE_BWD, rj.pre_bwd_args(t2["s0"], t2["s1"], KH, RW0, RW1, dh2))], dout)
    torch.cuda.synchronize(dev)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(dh2, dh1), "d hray of the rgb head"
    # the reduced weight gradients: one range of partial blocks -> one addend per target, bit for bit; else both within the fp64 bound
    ref, mag = _reduce_reference(cap, ws2, {x.data_ptr(): x0 for x, x0 in zip(tgt2, init)})
    for a, b, name in zip(tgt1, tgt2, ("dW0", "dW1", "dW2", "db2")):
        if cap.n_blocks < 16:
            assert torch.equal(a, b), name
        for side, x in (("stand-alone", a), ("job", b)):
            w, m = ref[b.data_ptr()], mag[b.data_ptr()]
            bound = (cap.n_blocks + 1) * 2.0 ** -24 * (m + w.abs()) + 1e-30
            err = (x.double() - w).abs()
            print(f"R={R} {name} {side}: max err {err.max().item():.3e}, max err/bound {(err / bound).max().item():.3f}")
            assert bool((err <= bound).all()), f"{name} ({side}): {(err / bound).max().item():.3f} x bound"


@pytest.mark.parametrize("R", [33, 257])
def test_pre_bwd_job_at_the_widest_input(hip_lib, R):
    """kh = n_hidden = 64 is the one shape whose LDS (49 280 B) lies above the 48 KiB that need no reservation: the job takes it as
    emer_ray_pre_bwd does, alone and as the second stage of the backward chain."""
    from emernerf_amd import _lib, ray_jobs as rj
    from emernerf_amd._lib import ACT_SIGMOID
    dev, K = _dev(), 64
    g = torch.Generator().manual_seed(64 + R)
    W0, W1, W2 = _rand(g, H, K, scale=0.2), _rand(g, H, H + K, scale=0.2), _rand(g, C, H, scale=0.2)
    dout, out, a1, a2 = _rand(g, R, C), torch.rand(R, C, generator=g).to(dev), _rand(g, R, H).relu(), _rand(g, R, H).relu()
    d2, d1, d0, dx = (torch.empty(R, w, device=dev) for w in (C, H, H, K))
    _lib.call("emer_ray_head_bwd", dout.data_ptr(), out.data_ptr(), a1.data_ptr(), a2.data_ptr(), R, W1.data_ptr(), W1.stride(0), W2.data_ptr(), C,
              ACT_SIGMOID, d2.data_ptr(), d1.data_ptr(), d0.data_ptr(), _st())
    _lib.call("emer_ray_pre_bwd", d0.data_ptr(), d1.data_ptr(), H, R, K, H, W0.data_ptr(), W0.stride(0), W1[:, H:].data_ptr(), W1.stride(0), dx.data_ptr(), K, _st())
    e2, e1, e0, ex, ey = (torch.full((R, w), float("nan"), device=dev) for w in (C, H, H, K, K))
    rj.launch([rj.bwd_chain_job(rj.head_bwd_args(dout, out, a1, a2, W1, W2, ACT_SIGMOID, e2, e1, e0), rj.pre_bwd_args(e0, e1, K, W0, W1, ex)),
               rj.job(rj.PRE_BWD, rj.pre_bwd_args(d0, d1, K, W0, W1, ey))], dout)
    torch.cuda.synchronize(dev)
    for name, a, b in (("dpre2", e2, d2), ("dpre1", e1, d1), ("dpre0", e0, d0), ("dx (chain)", ex, dx), ("dx (job)", ey, dx)):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("n_emb", [3, 7])
@pytest.mark.parametrize("R", ROWS)
def test_launch_b_embedding_gradient_equals_embed_grad(hip_lib, R, n_emb):
    """The embedding table's gradient as a job: deterministic, bit for bit emer_embed_grad, the unused row exactly as it was."""
    from emernerf_amd import _lib, ray_jobs as rj
    c, _ = _shared(R, n_emb)
    g = torch.Generator().manual_seed(R + n_emb)
    ga, gb = _rand(g, R, KH), _rand(g, R, KH)
    dw0 = _rand(g, n_emb, E)
    want, got = dw0.clone(), dw0.clone()
    _lib.call("emer_embed_grad", ga[:, P:].data_ptr(), KH, gb[:, P:].data_ptr(), KH, c["idx"].data_ptr(), 1, R, n_emb, E, want.data_ptr(), _st())
    rj.launch([rj.job(rj.EMBED_GRAD, rj.embed_grad_args(ga[:, P:], KH, gb[:, P:], KH, c["idx"], n_emb, E, got))], ga)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got[n_emb - 1], dw0[n_emb - 1]), "no ray uses the last row"
    used = int(c["idx"][0])
    assert not torch.equal(got[used], dw0[used])


def _wgrad_jobs(c, fwd, bwd, s0, s1, targets):
    """The five per-ray weight-gradient jobs of a static step: the sky head's three layers, the rgb head's two per-ray blocks."""
    tw2, tb2, tw1, tb1, tw0, tb0, rw1, rb1, rw0, rb0 = targets
    x, h = fwd["out_sky"], fwd["out_rgb"]
    sky = [(bwd["dpre2"], [(fwd["a2"], H, 0)], tw2, tb2), (bwd["dpre1"], [(fwd["a1"], H, 0), (x, KH, H)], tw1, tb1), (bwd["dpre0"], [(x, KH, 0)], tw0, tb0)]
    rgb = [(s1, [(h, KH, H)], rw1, rb1), (s0, [(h, KH, 0)], rw0, rb0)]
    return sky, rgb


@pytest.mark.parametrize("preload", [False, True])
@pytest.mark.parametrize("R", ROWS)
def test_launch_b_wgrad_jobs_equal_ray_wgrad(hip_lib, R, preload):
    """All five ray_wgrad jobs in one launch.  Up to 256 rows every target receives one addend: bit for bit emer_ray_wgrad, onto zeroed
    targets and onto targets that hold a value.  Beyond, the chunks' atomics arrive in any order on either side: both against fp64 with
    the bound of test_ray_wgrad_matches_fp64."""
    from emernerf_amd import fused, ray_jobs as rj
    c, fwd = _shared(R)
    dev = _dev()
    g = torch.Generator().manual_seed(7 * R + preload)
    bwd = _sky_backward_standalone(c, fwd, _rand(g, R, C))
    s0, s1 = _rand(g, R, H), _rand(g, R, H)
    shapes = [(C, H), (C,), (H, H + KH), (H,), (H, KH), (H,), (H, H + KH + 64), (H,), (H, KH + 64), (H,)]
    init = [(_rand(g, *s) if preload else torch.zeros(*s, device=dev)) for s in shapes]
    want, got = [x.clone() for x in init], [x.clone() for x in init]
    sky, rgb = _wgrad_jobs(c, fwd, bwd, s0, s1, want)
    fused.ray_wgrad(sky, s0)
    fused.ray_wgrad(rgb, s0)
    sky, rgb = _wgrad_jobs(c, fwd, bwd, s0, s1, got)
    rj.launch([rj.wgrad_job(*j) for j in sky + rgb], s0)
    torch.cuda.synchronize(dev)
    if R <= 256:
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"target {i}"
        return
    ref = [x.double().clone() for x in init]
    sky, rgb = _wgrad_jobs(c, fwd, bwd, s0, s1, ref)
    for dy, blocks, dw, db in sky + rgb:
        for xb, width, dst in blocks:
            dw[:, dst:dst + width] += dy.double().T @ xb[:, :width].double()
        db += dy.double().sum(0)
    for i, (a, b, w) in enumerate(zip(got, want, ref)):
        for side, x in (("job", a), ("stand-alone", b)):
            err = (x.double() - w).abs().max().item()
            assert err <= 2e-6 * max(1.0, w.abs().max().item()), f"target {i} ({side}): {err:.3e}"


@pytest.mark.parametrize("R", [33, 600])
def test_job_list_edges(hip_lib, R):
    """A list of one kind only, and a full list (EMER_RAY_JOBS_MAX independent jobs, one of every single-stage kind but the reduction),
    equal the stand-alone launches; an over-long or empty list is refused."""
    from emernerf_amd import _lib, fused, ray_jobs as rj
    from emernerf_amd._lib import ACT_SIGMOID, EmerError
    c, fwd = _shared(R)
    dev = _dev()
    g = torch.Generator().manual_seed(R)
    W0, B0, W1, B1, W2, B2 = c["sky"]
    RW0, RB0, RW1, RB1 = c["rgb"]
    nan = lambda t: torch.full_like(t, float("nan"))
    # one kind: the two pre_fwd of a step
    rb_rgb, rb_sky = nan(fwd["rb_rgb"]), nan(fwd["rb_sky"])
    rj.launch([rj.job(rj.PRE_FWD, rj.pre_fwd_args(fwd["out_rgb"], RW0, RB0, RW1, RB1, rb_rgb)),
               rj.job(rj.PRE_FWD, rj.pre_fwd_args(fwd["out_sky"], W0, B0, W1, B1, rb_sky))], rb_rgb)
    torch.cuda.synchronize(dev)
    assert torch.equal(rb_rgb, fwd["rb_rgb"]) and torch.equal(rb_sky, fwd["rb_sky"])
    # the full list
    dout = _rand(g, R, C)
    bwd = _sky_backward_standalone(c, fwd, dout)
    ga, gb = _rand(g, R, KH), _rand(g, R, KH)
    dwe_want = torch.zeros(c["n_emb"], E, device=dev)
    _lib.call("emer_embed_grad", ga[:, P:].data_ptr(), KH, gb[:, P:].data_ptr(), KH, c["idx"].data_ptr(), 1, R, c["n_emb"], E, dwe_want.data_ptr(), _st())
    wg_want, wb_want = torch.zeros(C, H, device=dev), torch.zeros(C, device=dev)
    small = slice(0, min(R, 256))   # one chunk: one addend per target
    fused.ray_wgrad([(bwd["dpre2"][small], [(fwd["a2"][small], H, 0)], wg_want, wb_want)], dout)
    o_rgb, o_sky, rb2, a1, a2, out = nan(fwd["out_rgb"]), nan(fwd["out_sky"]), nan(fwd["rb_rgb"]), nan(fwd["a1"]), nan(fwd["a2"]), nan(fwd["out"])
    d2, d1, d0, dx = nan(bwd["dpre2"]), nan(bwd["dpre1"]), nan(bwd["dpre0"]), nan(bwd["dx"])
    dwe, wg, wb = torch.zeros_like(dwe_want), torch.zeros_like(wg_want), torch.zeros_like(wb_want)
    jobs = [rj.job(rj.INPUTS, rj.inputs_args(c["dirs"], c["idx"], c["emb"], MAX_DEG, o_rgb, None)),
            rj.job(rj.INPUTS, rj.inputs_args(c["dirs"], c["idx"], c["emb"], MAX_DEG, None, o_sky)),
            rj.job(rj.PRE_FWD, rj.pre_fwd_args(fwd["out_rgb"], RW0, RB0, RW1, RB1, rb2)),
            rj.job(rj.HEAD_FWD, rj.head_fwd_args(fwd["rb_sky"], W1, W2, B2, ACT_SIGMOID, a1, a2, out)),
            rj.job(rj.HEAD_BWD, rj.head_bwd_args(dout, fwd["out"], fwd["a1"], fwd["a2"], W1, W2, ACT_SIGMOID, d2, d1, d0)),
            rj.job(rj.PRE_BWD, rj.pre_bwd_args(bwd["dpre0"], bwd["dpre1"], KH, W0, W1, dx)),
            rj.wgrad_job(bwd["dpre2"][small], [(fwd["a2"][small], H, 0)], wg, wb),
            rj.job(rj.EMBED_GRAD, rj.embed_grad_args(ga[:, P:], KH, gb[:, P:], KH, c["idx"], c["n_emb"], E, dwe))]
    assert len(jobs) == rj.MAX_JOBS
    rj.launch(jobs, dout)
    torch.cuda.synchronize(dev)
    for name, a, b in (("out_rgb", o_rgb, fwd["out_rgb"]), ("out_sky", o_sky, fwd["out_sky"]), ("rb", rb2, fwd["rb_rgb"]), ("a1", a1, fwd["a1"]),
                       ("a2", a2, fwd["a2"]), ("out", out, fwd["out"]), ("dpre2", d2, bwd["dpre2"]), ("dpre1", d1, bwd["dpre1"]),
                       ("dpre0", d0, bwd["dpre0"]), ("dx", dx, bwd["dx"]), ("dW2", wg, wg_want), ("db2", wb, wb_want), ("d emb", dwe, dwe_want)):
        assert torch.equal(a, b), name
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    arr = (rj.RayJob * (rj.MAX_JOBS + 1))(*(jobs + jobs[:1]))
    with pytest.raises(EmerError):
        _lib.call("emer_ray_jobs", arr, rj.MAX_JOBS + 1, st)
    with pytest.raises(EmerError):
        _lib.call("emer_ray_jobs", arr, 0, st)
