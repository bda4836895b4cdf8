"""The three job launches of a static step (ray_jobs: the front launch, launch A, launch B) against the separate launches, on whole
training steps: two trainers from one seed, the switch on and off.  256 rays x 32 samples, so that every atomic target of ray_wgrad
receives one addend (one 256-row chunk) and the per-ray gradients are reproducible on both sides.

What is compared how:
  * the loss, and .grad of every parameter of the two per-ray heads and of the embedding table: bit for bit -- except the four
    tensors that the rgb backward's partials are reduced into (rgb head W0, W1, W2, b2).  At 256 rays that kernel leaves 64 partials,
    which the reduction (stand-alone or as a job) cuts into 8 ranges whose sums meet in relaxed float atomics: the order of the 8
    addends is not fixed on EITHER side, so bit equality cannot be asked of them.  They are held to the bound that
    test_a_metric_shape_gpu.py uses for two launches of an order-dependent sum, 1e-6 x the largest entry;
  * the hash tables' gradients: that same bound (their backward is untouched; it reads dgeo, which is bit-equal).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

RAYS, SAMPLES, PROP = 256, 32, (32, 16)
ATOMIC_SUMS = ("rgb_head.layers.0.weight", "rgb_head.layers.1.weight", "rgb_head.layers.2.weight", "rgb_head.layers.2.bias")


@pytest.fixture(autouse=True)
def _restore_switch():
    from emernerf_amd import ray_jobs
    prev = ray_jobs.ENABLED
    yield
    ray_jobs.ENABLED = prev


def _step_of_kind(prop: bool, start: int = 1000) -> int:
    """The first iteration >= start that trains (or does not train) the proposal nets, by the trainer's own schedule."""
    from emernerf_amd.prop_net import get_proposal_requires_grad_fn
    fn = get_proposal_requires_grad_fn()
    for s in range(start + 64):
        v = bool(fn(s))
        if s >= start and v == prop:
            return s
    raise AssertionError("no such step")


def _one_step(switch: bool, prop: bool, use_graph: bool, kind: str = "static", freeze_embedding: bool = False, drop=()):
    """loss and gradients of ONE step of a fresh trainer (seeded), with the switch set for its whole life."""
    from emernerf_amd import ray_jobs
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    ray_jobs.ENABLED = switch
    tr = Trainer(kind=kind, device=dev, num_samples=SAMPLES, prop_samples=PROP, table_init=0.3, seed=11, use_graph=use_graph)
    if freeze_embedding:
        tr.model.appearance_embedding.weight.requires_grad_(False)
    tr.set_step(_step_of_kind(prop))
    tail_ok = tr._ray_tail_ok()   # (while the switch is as this trainer runs)
    data = {k: v for k, v in synthetic_rays(RAYS, dev, seed=5).items() if k not in drop}
    enqueued = []
    orig = ray_jobs.enqueue
    ray_jobs.enqueue = lambda *a, **kw: (enqueued.append(1), orig(*a, **kw))[1]
    try:
        out = tr.train_step(data)
    finally:
        ray_jobs.enqueue = orig
    torch.cuda.synchronize(dev)
    assert bool(out["prop_grad"]) == prop
    assert tr.use_graph == use_graph, "the capture fell back to eager launches"
    assert ray_jobs.pending() == 0 and not ray_jobs.armed(), "a job was left in the queue"
    grads = {n: p.grad.detach().clone() for n, p in tr.model.named_parameters() if p.grad is not None}
    return dict(loss=out["loss"].detach().clone() if torch.is_tensor(out["loss"]) else out["loss"], grads=grads, enqueued=len(enqueued), trainer=tr, tail_ok=tail_ok)


def _compare(on, off, what, min_checked=14):
    assert torch.equal(torch.as_tensor(on["loss"]), torch.as_tensor(off["loss"])), f"{what}: loss {on['loss']} vs {off['loss']}"
    assert on["grads"].keys() == off["grads"].keys()
    checked = 0
    for name, want in off["grads"].items():
        got = on["grads"][name]
        head = name.startswith(("rgb_head.", "sky_head.", "appearance_embedding."))
        table = name.endswith("tcnn_encoding.params")
        if not (head or table):
            continue
        d = (got - want).abs().max().item()
        scale = want.abs().max().item()
        print(f"{what}: {name}: max |on - off| = {d:.3e} (largest entry {scale:.3e})")
        if head and name not in ATOMIC_SUMS:
            assert torch.equal(got, want), f"{what}: {name}: max diff {d:.3e}"
        else:
            assert d <= 1e-6 * scale, f"{what}: {name}: {d:.3e} vs {1e-6 * scale:.3e}"
        checked += 1
    assert checked >= min_checked   # 6 + 6 head tensors, the embedding, the table


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("prop", [True, False], ids=["prop_step", "plain_step"])
def test_static_step_equals_the_separate_launches(hip_lib, prop, use_graph):
    on = _one_step(True, prop, use_graph)
    off = _one_step(False, prop, use_graph)
    assert on["tail_ok"] and on["enqueued"] == 2 * (3 if use_graph else 1), "both heads defer their per-ray jobs, once per forward+backward"
    assert off["enqueued"] == 0
    _compare(on, off, f"static prop={prop} graph={use_graph}")


def test_frozen_embedding_leaves_no_job_unflushed(hip_lib):
    """When the embedding takes no gradient nobody calls the per-ray inputs' backward: the trainer's own flush runs the queue."""
    on = _one_step(True, False, False, freeze_embedding=True)
    off = _one_step(False, False, False, freeze_embedding=True)
    assert on["enqueued"] == 2
    assert "appearance_embedding.weight" not in on["grads"] or float(on["grads"]["appearance_embedding.weight"].abs().max()) == 0.0
    _compare(on, off, "frozen embedding", min_checked=13)


def test_rows_without_indices_take_the_immediate_path(hip_lib):
    """A batch without per-ray embedding indices: the heads' rows are a torch cat of the direction encoding and the mean embedding,
    not outputs of the per-ray inputs Function.  Their gradients go to torch nodes that read them at once, so although the trainer
    arms the queue for the static model, neither head may defer: nothing is enqueued and the step equals the switch-off step."""
    on = _one_step(True, False, False, drop=("img_idx", "cam_idx"))
    off = _one_step(False, False, False, drop=("img_idx", "cam_idx"))
    assert on["tail_ok"], "the queue is armed for the static model"
    assert on["enqueued"] == 0
    assert float(on["grads"]["appearance_embedding.weight"].abs().max()) > 0.0
    _compare(on, off, "no indices")


def _dp_worker(rank, port):
    """One rank with EMER_DP_FORCE=1 (the trainer's data-parallel path on a communicator of one): gradient buckets are launched from
    inside the backward, so the tail must stay off; the front launch may run."""
    import os
    import torch.distributed as dist
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ["EMER_DP_FORCE"] = "1"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        for prop in (True, False):
            on = _one_step(True, prop, False)
            off = _one_step(False, prop, False)
            assert on["trainer"]._dp_on and not on["tail_ok"]
            assert on["enqueued"] == 0, "a head deferred its jobs in a data-parallel step"
            _compare(on, off, f"data-parallel prop={prop}")
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_keeps_the_tail_off(hip_lib):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mp.spawn(_dp_worker, args=(port,), nprocs=1, join=True)


def test_dynamic_step_takes_the_immediate_path(hip_lib):
    """The per-ray rows of a dynamic model feed two rgb heads: autograd adds their gradients before the rows' producer sees them, so
    the tail must not be armed there (the front launch may run).  The step equals the one with the switch off."""
    on = _one_step(True, False, False, kind="dynamic")
    off = _one_step(False, False, False, kind="dynamic")
    assert on["enqueued"] == 0 and not on["tail_ok"]
    _compare(on, off, "dynamic")


def test_single_consumer_is_asserted(hip_lib):
    """Arming the tail by hand on a model whose rows have two consumers is caught where the gradients meet."""
    from emernerf_amd import ray_jobs
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    ray_jobs.ENABLED = True
    tr = Trainer(kind="dynamic", device=dev, num_samples=SAMPLES, prop_samples=PROP, table_init=0.3, seed=11)
    tr.set_step(_step_of_kind(False))
    tr._ray_tail_ok = lambda: True
    with pytest.raises(RuntimeError, match="more than one consumer"):
        tr.train_step(synthetic_rays(RAYS, dev, seed=5))
    torch.cuda.synchronize(dev)
    assert not ray_jobs.armed()


def _count_launches(tr, data):
    from torch.profiler import ProfilerActivity, profile
    while tr.requires_grad_fn.since_last >= 5:   # profile a step that does not train the proposal nets (5 in 6 steps)
        tr.train_step(data)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = tr.train_step(data)
        torch.cuda.synchronize()
    assert not out["prop_grad"]
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.device_time_total > 0]
    return [e.name for e in kernels if "Memcpy" not in e.name and "Memset" not in e.name]


def test_static_step_launch_count(hip_lib):
    """Counted as test_flow_step_launch_budget counts: a static step that does not train the proposal nets has at least 8 launches
    fewer with the switch on (11 per-ray launches become 3), and none of the per-ray kernels runs on its own."""
    from emernerf_amd import ray_jobs
    from emernerf_amd.trainer import Trainer, synthetic_rays
    dev = torch.device("cuda:0")
    data = synthetic_rays(RAYS, dev, seed=1)
    names = {}
    for switch in (False, True):
        ray_jobs.ENABLED = switch
        tr = Trainer(kind="static", device=dev, num_samples=SAMPLES, prop_samples=PROP, seed=3)
        tr.set_step(1000)
        for _ in range(2):
            tr.train_step(data)
        names[switch] = _count_launches(tr, data)
    off, on = names[False], names[True]
    print(f"launches: off {len(off)}, on {len(on)}")
    gone = ("ray_inputs_kernel", "ray_pre_", "ray_head_", "ray_wgrad_kernel", "embed_grad_kernel")
    assert sum(any(g in n for g in gone) for n in off) == 10, "the separate launches: inputs, 2 pre_fwd, head_fwd, head_bwd, 2 pre_bwd, 2 wgrad, embed_grad"
    assert not [n for n in on if any(g in n for g in gone)], "a per-ray kernel ran on its own with the switch on"
    assert sum("ray_jobs_" in n for n in on) == 3
    assert len(on) <= len(off) - 8, f"{len(off)} -> {len(on)} launches"
