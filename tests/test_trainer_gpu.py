"""Trainer-level checks on the GPU: hipGraph replay of a step == eager launches; gradient sinks == autograd accumulation."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _make(use_graph):
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    tr = Trainer(kind="static", device=dev, num_samples=32, prop_samples=(32, 16), table_init=0.3, seed=3, use_graph=use_graph)
    jit = torch.full((512,), 0.37, device=dev)
    tr.estimator.jitter_fn = lambda n, d: jit  # deterministic stratified jitter: both runs see identical samples
    return tr, synthetic_rays(512, dev, seed=5)


def _params_agree(pe, pg, steps: int, lr: float = 0.01) -> None:
    """Parameters of two runs of the same steps (eager launches / hipGraph replay).  The runs differ by summation order (float atomics in
    the weight-gradient reductions), and Adam turns a gradient that is zero up to that noise into a +-lr step: a FEW entries may differ by
    ~2 lr per step.  Anything systematic -- a constant read from freed memory corrupts the sample positions of whole rays -- moves
    thousands of table entries instead."""
    diff = (pe - pg).abs()
    tol = 2e-4 * float(pe.abs().max())
    n_bad = int((diff > tol).sum())
    assert n_bad <= max(10, pe.numel() // 100000), f"{n_bad} of {pe.numel()} parameters differ by more than {tol:.2e} (max {float(diff.max()):.3e})"
    assert float(diff.max()) <= 2 * lr * steps + tol, f"max difference {float(diff.max()):.3e} exceeds {steps} steps' worth of sign flips"


def test_graph_replay_equals_eager(hip_lib):
    """Seven optimizer steps (both step types: with and without proposal-net training) with the forward+backward replayed
    from captured hipGraphs give the same parameters as eager launches (fp32 atomics order aside)."""
    eager, data = _make(False)
    graph, _ = _make(True)
    for tr in (eager, graph):
        tr.step_count = 0
    le, lg = [], []
    for _ in range(7):
        le.append(float(eager.train_step(data)["loss"]))
        lg.append(float(graph.train_step(data)["loss"]))
    assert graph.use_graph and len(graph._graphs) == 2, "both step types must have been captured"
    assert max(abs(a - b) for a, b in zip(le, lg)) < 1e-5 * max(abs(v) for v in le)
    _params_agree(eager.flat.params, graph.flat.params, steps=6)


def test_finite_check_works_under_graph_replay(hip_lib, monkeypatch):
    """EMER_CHECK_FINITE=1 with the default launch mode: the check cannot read the host inside a capture, so its verdict stays on
    the device and is read after every replay; a non-finite pixel (hence a non-finite gradient entering the grid backward) raises."""
    from emernerf_amd import ops
    monkeypatch.setattr(ops, "CHECK_FINITE", True)
    tr, data = _make(True)
    for _ in range(3):
        tr.train_step(data)
    assert tr.use_graph and tr._graphs, "the step must be replayed from a graph"
    assert all(len(v[2]) >= 1 for v in tr._graphs.values()), "the capture must have recorded the deferred checks"
    bad = {k: v.clone() for k, v in data.items()}
    bad["pixels"][7, 1] = float("inf")
    with pytest.raises(FloatingPointError, match="hash-grid backward"):
        for _ in range(2):
            tr.train_step(bad)


def test_graph_step_survives_a_render_with_another_ray_count(hip_lib):
    """a captured step graph has the address of the sampler's level-0 histogram baked in; an evaluation chunk or a lidar
    step with another ray count on the same estimator must not free or replace that tensor.  graph step, render 100 rays, graph
    step == the same three calls with eager launches."""
    from emernerf_amd.render_utils import render_rays
    from emernerf_amd.trainer import synthetic_rays
    eager, data = _make(False)
    graph, _ = _make(True)
    other = synthetic_rays(100, torch.device("cuda:0"), seed=9)
    for tr in (eager, graph):
        tr.set_step(1000)
    jit100 = torch.full((100,), 0.37, device="cuda:0")
    jit512 = torch.full((512,), 0.37, device="cuda:0")
    for tr in (eager, graph):
        tr.estimator.jitter_fn = lambda n, d: jit512 if n == 512 else jit100
        for _ in range(3):
            tr.train_step(data)
        with torch.no_grad():
            render_rays(radiance_field=tr.model, proposal_estimator=tr.estimator, proposal_networks=tr.props, data_dict=other, cfg=tr.rcfg)
        # churn the allocator: if the constant had been freed, this is where its memory would be reused
        junk = [torch.full((512, 2), 7.0, device="cuda:0") for _ in range(64)]
        for _ in range(3):
            tr.train_step(data)
        del junk
    assert graph.use_graph
    _params_agree(eager.flat.params, graph.flat.params, steps=6)


def test_render_pixels_loop(hip_lib):
    """emernerf_amd.video_utils.render_pixels (reference: radiance_fields/video_utils.py:50-468) over a synthetic split:
    reference key names, image shapes, chunked rendering == one-shot rendering of the same rays."""
    import numpy as np
    from emernerf_amd.pixel_source import PixelSource
    from emernerf_amd.render_utils import render_rays
    from emernerf_amd.trainer import Trainer, render_config
    from emernerf_amd.video_utils import render_pixels
    dev = torch.device("cuda:0")
    tr = Trainer(kind="dynamic", device=dev, num_samples=32, prop_samples=(32, 16), table_init=0.3, seed=2)
    src = PixelSource.synthetic(dev, num_imgs=4, height=24, width=40, seed=1)
    cfg = render_config(32, (32, 16), chunk=256)  # 960 rays per image -> 4 chunks
    out = render_pixels(cfg, tr.model, tr.estimator, src, proposal_networks=tr.props, compute_metrics=True, vis_indices=[0, 2])
    for k in ("rgbs", "gt_rgbs", "depths", "opacities", "static_rgbs", "dynamic_rgbs", "static_depths", "dynamic_depths",
              "static_opacities", "dynamic_opacities", "shadow_reduced_static_rgbs", "shadow_only_static_rgbs", "gt_sky_masks"):
        assert k in out and len(out[k]) == 2, k
    assert out["rgbs"][0].shape == (24, 40, 3) and out["depths"][0].shape == (24, 40) and np.isfinite(out["psnr"])
    assert out["render_rays_per_s"] > 0
    big = render_config(32, (32, 16), chunk=1 << 20)
    with torch.no_grad():
        one = render_rays(radiance_field=tr.model, proposal_estimator=tr.estimator, proposal_networks=tr.props, data_dict=src[2],
                          cfg=big, return_decomposition=True)
    np.testing.assert_allclose(out["rgbs"][1], one["rgb"].cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["depths"][1], one["depth"].squeeze(-1).cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_lidar_step_runs_and_matches_oracle_gradients(hip_lib, oracle):
    """Trainer.lidar_step (train_emernerf.py:747-826): density-only render of lidar rays + depth / line-of-sight losses;
    gradients vs oracle/ref_path.py with the losses restated in torch."""
    import math
    import numpy as np
    from oracle.ref_path import prop_loss
    from emernerf_amd import fused
    from emernerf_amd.render_utils import render_rays
    from emernerf_amd.trainer import Trainer, synthetic_lidar_rays
    from tests.test_a_metric_shape_gpu import _ref_from_trainer
    dev = torch.device("cuda:0")
    R, S = 768, 64
    tr = Trainer(kind="static", device=dev, num_samples=S, prop_samples=(64, 32), table_init=0.3, seed=4)
    tr.step_count = 4000  # line of sight active: eps = 6 - 3.5 * 2000 / 23000, coefficient 0.1
    ref = _ref_from_trainer(oracle, tr)
    data = synthetic_lidar_rays(R, dev, seed=3)
    cpu = {k: v.cpu() for k, v in data.items()}
    g = torch.Generator().manual_seed(1)
    jit = [torch.rand(R, generator=g) for _ in range(3)]
    it = iter([j.to(dev) for j in jit])
    tr.estimator.jitter_fn = lambda n, d: next(it)
    tr.flat.zero_grad()
    with fused.grad_sinks(True):
        res = render_rays(radiance_field=tr.model, proposal_estimator=tr.estimator, proposal_networks=tr.props, data_dict=data,
                          cfg=tr.rcfg, proposal_requires_grad=False, prefix="lidar_")
        loss_hip = tr.lidar_losses(res, data, 4000)
        (loss_hip * 1024.0).backward()
    tr.flat.finish_grads("main")
    torch.cuda.synchronize()
    assert set(res) - {"extras"} == {"depth", "opacity", "median_depth"}
    r = ref.render_rays(cpu, S, [64, 32], jitters=jit, requires_grad=False, prefix="lidar_")
    gt = cpu["lidar_ranges"].squeeze(-1)
    eps = 6.0 + (2.5 - 6.0) / (25000 - 2000) * (4000 - 2000)
    valid = (gt > 0.01) & (gt < 80)
    nd = lambda v: torch.clamp(v / 80.0, 0.0, 1.0)  # noqa: E731
    depth_loss = ((nd(r["depth"].squeeze(-1)[valid]) - nd(gt[valid])) ** 2).mean()
    w, t = r["extras"]["weights"], r["extras"]["t_vals"]
    gd = gt[:, None]
    sigma = eps / 3
    delta = (1 / math.sqrt(2 * math.pi * sigma ** 2)) * torch.exp(-((t - gd) ** 2) / (2 * sigma ** 2))
    sight = ((w.square() * (t < gd - eps)).sum(-1, keepdim=True).mean()
             + ((w - delta).square() * ((t > gd - eps) & (t < gd + eps))).sum(-1, keepdim=True).mean())
    loss = depth_loss + 0.1 * (sight * (gt > 0)).mean()
    (loss * 1024.0).backward()
    np.testing.assert_allclose(float(loss_hip), float(loss), rtol=1e-4)
    for k in ("xyz_encoder.tcnn_encoding.params", "base_mlp.0.weight", "base_mlp.2.weight"):
        want = ref.t["model/" + k].grad
        got = dict(tr.model.named_parameters())[k].grad.cpu()
        assert float((got - want).abs().max()) <= 2e-3 * float(want.abs().max()), k
    # and the whole step runs (second optimizer step of an iteration)
    p0 = tr.flat.params.clone()
    tr.estimator.jitter_fn = lambda n, d: torch.rand(n, device=d)
    out = tr.lidar_step(synthetic_lidar_rays(R, dev, seed=5))
    assert torch.isfinite(out["loss"]) and not torch.equal(p0, tr.flat.params)


@pytest.mark.parametrize("kind", ["dynamic", "flow", "feature"])
def test_other_configs_step(hip_lib, kind):
    """BASELINE configs[2..4] take optimizer steps on the fused path (dynamic + shadow, flow, flow + feature head + PE)."""
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    tr = Trainer(kind=kind, device=dev, num_samples=32, prop_samples=(32, 16), table_init=0.2, seed=1)
    kw = dict(num_cams=3, feature_dim=64) if kind == "feature" else {}
    data = synthetic_rays(512, dev, seed=3, **kw)
    l0 = float(tr.train_step(data)["loss"])
    for _ in range(6):
        l1 = float(tr.train_step(data)["loss"])
    assert torch.isfinite(torch.tensor([l0, l1])).all() and l1 < l0


def test_table_gradient_fallbacks_honour_the_unzeroed_grad_contract(hip_lib, monkeypatch):
    """FlatParams.zero_grad does not zero table gradients (the owner-computes backward overwrites them).  A table gradient
    that comes back through autograd instead -- the global-atomics path when the sliced kernel does not cover a grid, fp16
    gradients, the row-major encoder -- must therefore clear the stale buffer itself (it was added onto last
    step's values and then zeroed, i.e. the table trained with a zero gradient).  Two backward passes on the same data
    without an optimizer step in between must give the same gradient both times, equal to the default path's."""
    from emernerf_amd import ops
    dflt, data = _make(False)

    def grads(tr):
        out = []
        for _ in range(2):
            tr._forward_backward(data, False)
            tr._exchange_grads(False)
            out.append(tr.flat.grads.clone())
        return out
    g_ref = grads(dflt)
    monkeypatch.setattr(ops, "sliced_supported", lambda desc: False)   # every table gradient now returns through autograd
    fb, _ = _make(False)
    g_fb = grads(fb)
    a, b = fb.flat.ranges["main"]
    scale = float(g_ref[0][a:b].abs().max())
    assert scale > 0
    assert float((g_fb[0][a:b] - g_fb[1][a:b]).abs().max()) <= 1e-5 * scale, "second backward saw stale table gradients"
    assert float((g_fb[0][a:b] - g_ref[0][a:b]).abs().max()) <= 2e-4 * scale
    assert float((g_ref[0][a:b] - g_ref[1][a:b]).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("use_graph", [False, True])
def test_tables_end_a_step_neither_fresh_nor_pending(hip_lib, use_graph):
    """The state a step leaves on its tables (emernerf_amd/table_grad.py): no evaluation pending on any table, and no table of a
    group the step trained still marked ``fresh`` -- its gradient was overwritten by a backward or zeroed by ``finish_grads``.
    (The tables of a group the step did NOT train -- the idle proposal net always, the trained one on the steps without proposal
    training -- keep the mark, as before the state objects: nothing wrote their gradient and nothing reads it.)  Three steps: without proposal training, with
    it, with it again; under ``use_graph`` the first two capture a graph each and the third only replays one, so none of the
    step's Python runs.  Then two backward passes on the same data without an optimizer step give the same gradient."""
    from emernerf_amd import table_grad
    tr, data = _make(use_graph)
    tr.step_count = 0
    assert len(tr.flat._tables) == 3 and all(getattr(p, "_emer_table", None) is not None for p in tr.flat._tables)
    kinds = []
    for _ in range(3):
        n_graphs = len(tr._graphs)
        out = tr.train_step(data)
        kinds.append((out["prop_grad"], len(tr._graphs) > n_graphs))
        trained = [tr.flat.ranges[g] for g in (("main", "prop") if out["prop_grad"] else ("main",))]
        for p, o in tr.flat._table_offsets:
            state = table_grad.of(p)
            assert state.pending_evals == 0
            if any(a <= o < b for a, b in trained):
                assert state.fresh is False, f"step {len(kinds)}: the table at {o} is still marked fresh"
            else:
                assert state.fresh is True, f"step {len(kinds)}: the table at {o} of a group the step did not train lost its mark"
    assert kinds == [(False, use_graph), (True, use_graph), (True, False)]
    grads = []
    for _ in range(2):
        tr._forward_backward(data, False)
        tr._exchange_grads(False)
        grads.append(tr.flat.grads.clone())
    a, b = tr.flat.ranges["main"]
    scale = float(grads[0][a:b].abs().max())
    assert scale > 0
    assert float((grads[0][a:b] - grads[1][a:b]).abs().max()) <= 1e-5 * scale, "the second backward saw the first one's table gradients"


def test_lr_schedule_ticks_twice_with_lidar_supervision(hip_lib):
    """scheduler.step() follows the pixel AND the lidar optimizer step in the reference (train_emernerf.py:745, :826)."""
    from emernerf_amd.trainer import synthetic_lidar_rays
    tr, data = _make(False)
    tr.train_step(data)
    assert tr.sched_ticks == 1 and tr.step_count == 1
    tr.estimator.jitter_fn = lambda n, d: torch.rand(n, device=d)
    tr.lidar_step(synthetic_lidar_rays(256, torch.device("cuda:0"), seed=2))
    assert tr.sched_ticks == 2 and tr.step_count == 1


@pytest.mark.parametrize("kind", ["flow", "feature"])
def test_batched_xyzt_evaluations_equal_call_by_call(hip_lib, monkeypatch, kind):
    """RadianceField._flow_branch_batched (one 3N-sample evaluation of the dynamic table, N + 2N of the flow table) gives the
    gradients of the call-by-call order of the reference (six evaluations, radiance_field.py:434-459,553-620)."""
    from emernerf_amd import radiance_field as RF
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    R, S = 384, 32
    kw = dict(num_cams=3, feature_dim=64) if kind == "feature" else {}
    data = synthetic_rays(R, dev, seed=8, **kw)
    g = torch.Generator().manual_seed(4)
    noise = torch.rand(R, S, 1, generator=g).to(dev)
    jit = [torch.rand(R, generator=g).to(dev) for _ in range(3)]
    grads = []
    for batched in (True, False):
        monkeypatch.setattr(RF, "BATCH_XYZT", batched)
        tr = Trainer(kind=kind, device=dev, num_samples=S, prop_samples=(32, 16), table_init=0.3, seed=6)
        it = iter(jit)
        tr.estimator.jitter_fn = lambda n, d: next(it)
        tr.model._noise = lambda like: noise
        loss = tr._forward_backward(data, prop_grad=True)
        tr._exchange_grads(True)
        grads.append((float(loss), tr.flat.grads.clone()))
    (la, ga), (lb, gb) = grads
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert float((ga - gb).abs().max()) <= 2e-4 * float(gb.abs().max())


def test_table_split_is_taken_by_the_last_backward_only(hip_lib):
    """The level cut of the data-parallel exchange (``TableGrad.split``) hands a range of the table's gradient to a collective while
    the rest is still being computed, so it may only be taken by a backward after which nothing writes that range again: the table's
    LAST backward of the step, writing the table's buffer directly.  One evaluation per step: the cut is taken and the range is final
    when the hook runs.  Two evaluations (warped positions, chunked training): the first backward to run is not the last one and the
    last one ADDS to what the first wrote -- no cut, the whole table goes with the late bucket."""
    from emernerf_amd import fused, ops, table_grad
    from emernerf_amd.tcnn_modules import Encoding
    dev = torch.device("cuda:0")
    enc = Encoding(3, dict(otype="HashGrid", n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16,
                           per_level_scale=1.3819)).to(dev)
    desc, tab = enc.desc, enc.params
    state = table_grad.of(tab, create=True)
    with torch.no_grad():
        tab.copy_(torch.rand_like(tab) - 0.5)
    assert ops.sliced_supported(desc)
    k = ops.sliced_split_level(desc)
    assert 0 < k < desc.n_levels
    g = torch.Generator().manual_seed(1)
    xa, xb = torch.rand(4096, 3, generator=g).to(dev), torch.rand(2048, 3, generator=g).to(dev)
    da, db = torch.randn(16, 4096, 2, generator=g).to(dev), torch.randn(16, 2048, 2, generator=g).to(dev)

    def run(with_hooks, two):
        tab.grad = torch.full_like(tab, float("nan"))   # the first backward of a step overwrites (no zero fill)
        state.begin_step()
        seen = []
        if with_hooks:
            state.on_last_backward = lambda: seen.append(("before",))
            state.split = (k, lambda p, lo, hi: seen.append(("split", tab.grad.view(-1)[lo:hi].clone(), lo, hi)))
        else:
            state.on_last_backward = state.split = None
        with fused.grad_sinks(True):
            loss = (ops.hashgrid_encode_lm(xa, tab, desc) * da).sum()
            if two:
                loss = loss + (ops.hashgrid_encode_lm(xb, tab, desc) * db).sum()
            loss.backward()
        torch.cuda.synchronize()
        return tab.grad.detach().clone().view(-1), seen
    try:
        for two in (False, True):
            ref, _ = run(False, two)
            got, seen = run(True, two)
            assert torch.isfinite(ref).all()
            assert float((ref - got).abs().max()) <= 1e-6 * float(ref.abs().max())
            kinds = [s[0] for s in seen]
            if two:
                assert kinds == ["before"], f"two evaluations: no level cut, one 'last backward' callback: {kinds}"
            else:
                assert kinds == ["before", "split"], f"one evaluation: both hooks, once each: {kinds}"
                _, at_hook, lo, hi = seen[1]
                assert (lo, hi) == (int(desc.offset[k]) * 2, tab.numel())
                assert float((at_hook - got[lo:hi]).abs().max()) == 0.0, "the level range was written after its collective would have started"
    finally:
        state.on_last_backward = state.split = None


def test_default_timestep_registration_takes_the_fused_warp(hip_lib):
    """``register_normalized_training_timesteps`` without ``time_diff`` leaves a 0-dim tensor (the reference's default route); the
    one-launch flow warp must be taken on that route too, with the same value as an explicit float."""
    from emernerf_amd import ops
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    tr = Trainer(kind="flow", device=dev, num_samples=16, prop_samples=(16, 8), table_init=0.3, seed=4)
    data = synthetic_rays(64, dev, seed=2)
    tr.model.register_normalized_training_timesteps(torch.linspace(0, 1, tr.cfg.num_train_timesteps))
    assert isinstance(tr.model.time_diff, torch.Tensor)
    calls, orig = [], ops.flow_warp

    def spy(*a, **kw):
        calls.append(a[5])
        return orig(*a, **kw)
    ops.flow_warp = spy
    try:
        tr.train_step(data)
    finally:
        ops.flow_warp = orig
    assert calls and all(isinstance(c, float) for c in calls), "the default registration must take the one-launch warp"
    assert abs(calls[0] - float(tr.model.time_diff)) == 0.0


def test_trainer_state_dict_is_a_snapshot_and_checks_the_layout(hip_lib):
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    tr = Trainer(kind="static", device=dev, num_samples=16, prop_samples=(16, 8), table_init=0.3, seed=5)
    data = synthetic_rays(64, dev, seed=3)
    tr.train_step(data)
    sd = tr.state_dict()
    m0 = sd["m"].clone()
    tr.train_step(data)
    assert torch.equal(sd["m"], m0), "state_dict must not alias the live moments"
    tr2 = Trainer(kind="static", device=dev, num_samples=16, prop_samples=(16, 8), table_init=0.3, seed=5)
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.m, m0) and tr2.step_count == 1 and tr2.loss_scale == tr.loss_scale and tr2.num_iters == tr.num_iters
    # the schedule length and the loss scale are the resuming run's (constructor), not the checkpoint's -- unless asked for
    tr4 = Trainer(kind="static", device=dev, num_samples=16, prop_samples=(16, 8), table_init=0.3, seed=5, num_iters=40000, loss_scale=512.0)
    with pytest.warns(UserWarning, match="keeping the constructor's"):
        tr4.load_state_dict(sd)
    assert tr4.num_iters == 40000 and tr4.loss_scale == 512.0 and tr4.step_count == 1
    tr4.load_state_dict(sd, restore_schedule=True)
    assert tr4.num_iters == tr.num_iters and tr4.loss_scale == tr.loss_scale
    bad = dict(sd)
    bad["ranges"] = {k: (a, b + 4) for k, (a, b) in sd["ranges"].items()}
    with pytest.raises(ValueError):
        tr2.load_state_dict(bad)
    # set_step replays the proposal schedule: the state k iterations leave behind
    tr3 = Trainer(kind="static", device=dev, num_samples=16, prop_samples=(16, 8), seed=5)
    fresh = type(tr3.requires_grad_fn)(tr3.requires_grad_fn.target, tr3.requires_grad_fn.num_steps)
    for s in range(1234):
        fresh(s)
    tr3.set_step(1234)
    assert tr3.requires_grad_fn.since_last == fresh.since_last and tr3.step_count == 1234


def test_flow_step_launch_budget(hip_lib):
    """A flow-model step at a 2048-ray shard is 87 kernel launches, 11 of them torch's (profiles/r05e_flow2048_step_sequence.txt; round 4:
    116 / 27).  The budget below leaves room for the profiler's own bookkeeping but not for a fusion coming undone (the cycle loss back on
    four slices: +9 torch launches; the plain heads back on streamed weight gradients: +15 launches)."""
    from torch.profiler import ProfilerActivity, profile
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    tr = Trainer(kind="flow", device=dev)
    tr.set_step(1000)
    data = synthetic_rays(2048, dev, seed=1)
    for _ in range(3):
        tr.train_step(data)
    while tr.requires_grad_fn.since_last >= 5:   # profile a step that does not train the proposal nets (5 in 6 steps)
        tr.train_step(data)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = tr.train_step(data)
        torch.cuda.synchronize()
    assert not out["prop_grad"]
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.device_time_total > 0]
    names = [e.name for e in kernels]
    ours = [n for n in names if n.startswith("emer::") or "emer::" in n]
    theirs = [n for n in names if n not in ours and "Memcpy" not in n and "Memset" not in n]
    assert len(ours) >= 60, "the HIP kernels must be the ones that run"
    assert len(names) <= 100, f"{len(names)} launches in a flow step"
    assert len(theirs) <= 14, f"{len(theirs)} torch launches in a flow step: {sorted(set(theirs))}"
