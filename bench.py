#!/usr/bin/env python3
"""Headline benchmark: train rays/s of the EmerNeRF hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 24 --warmup 6 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one full optimizer step on one synthetic ray batch per rank (BASELINE.json configs[1]: static-only
RadianceField, HashEncoder defaults D3/L16/F2/T2^19, 8192 rays x 128 samples, proposal rounds of 128 and 64):
proposal sampling -> field -> compositing -> losses -> backward -> (gradient exchange over RCCL: up to three buckets
of the flat gradient buffer, two of them hidden behind the backward) -> fused Adam.  Inputs (rays, parameters) are resident in HBM before the timed region.  Weak scaling:
every rank draws its own 8192 rays; value = world * rays * steps / max-over-ranks(time).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the headline fields (metric, value,
unit, higher_is_better, dtype, ms_per_step and what the same timed steps give for free: per-step spread, config).  --full adds
everything that takes passes of its own after the timed region: the other launch mode, the instrumented per-kernel breakdown and
the rooflines built on it, the CPU baseline with render parity, the lidar step and eval render, the trained-like and fp16-table
states and the secondary configs (the --no-* options skip single parts of it).  --dump-outputs DIR writes what the timed
path computes: the last timed step taken once more from the seeded parameters (dump_outputs).
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 matrix peak (MI355X_MICROARCH.md); the heads run exact 3-term bf16 splits on it
FP32_MFMA_PEAK_TFLOPS = 157.3   # dense fp32-input matrix peak, for reference (round 2 ran the heads on it)
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)
N_BATCHES = 8  # seeded ray batches rotated through the steps (a new batch every step)
PROP_SHAPE = (3, 8, 1)  # (D, L, F) of the proposal networks' grids (configs/default_config.yaml:51-58)


def grid_alg_bytes(D, L, F, sp=4, so=4, sg=4):
    """Algorithmic bytes per sample: fwd, bwd_params."""
    fwd = 4 * D + (2 ** D) * L * F * sp + L * F * so
    bwd = 4 * D + L * F * so + 2 * (2 ** D) * L * F * sg
    return fwd, bwd


def grid_roofline(timer, shape, steps: int, fwd_names=("emer_hashgrid_fwd", "emer_hashgrid_fwd_jac"),
                  bwd_names=("emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add", "emer_hashgrid_bwd_params_sliced_levels")):
    """HBM roofline of the grid launches of shape (D, L, F) recorded by ``timer`` over ``steps`` steps: achieved = SURVEY 8(d)'s
    algorithmic bytes per sample x the samples every launch really processed (``timer.ns``) / the summed launch durations."""
    us, tags, ns = timer.elapsed_us(), timer.tags, timer.ns
    D, L, F = shape
    fb, bb = grid_alg_bytes(D, L, F)

    def pick(names):
        t, n, k = 0.0, 0, 0
        for nm in names:
            for u, tg, cnt in zip(us.get(nm, []), tags.get(nm, []), ns.get(nm, [])):
                if tg == shape and cnt:
                    t, n, k = t + u, n + cnt, k + 1
        return t, n, k
    (tf, nf, kf), (tb, nb, kb) = pick(fwd_names), pick(bwd_names)
    if not kf:
        return None
    out = {"grid": f"D{D}/L{L}/F{F}", "bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s",
           "algorithmic_bytes_per_sample": {"fwd": fb, "bwd": bb},
           "launches_per_step": {"fwd": kf / steps, "bwd": kb / steps}, "ms_per_step": {"fwd": tf / 1e3 / steps, "bwd": tb / 1e3 / steps},
           "samples_per_step": {"fwd": nf / steps, "bwd": nb / steps},
           "achieved_fwd": fb * nf / (tf * 1e-6) / 1e9, "frac_fwd": fb * nf / (tf * 1e-6) / 1e9 / HBM_PEAK_GBPS}
    if kb:
        out.update({"achieved_bwd": bb * nb / (tb * 1e-6) / 1e9, "frac_bwd": bb * nb / (tb * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                    "frac_encode_plus_bwd_per_sample": (fb + bb) / ((tf / nf + tb / nb) * 1e-6) / 1e9 / HBM_PEAK_GBPS})
    return out


def cpu_baseline(trainer, rays: int, samples: int, steps: int = 12):
    """Oracle port (oracle/ref_path.py on the C oracle) timed on this box's host cores, bounded sample."""
    from oracle.train_parity import cotrain, ref_from_trainer
    from emernerf_amd.trainer import synthetic_rays
    cores = min(os.cpu_count() or 1, 32)  # more threads only add torch/OpenMP overhead at this sample size
    torch.set_num_threads(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    ref = ref_from_trainer(trainer)
    data = synthetic_rays(rays, "cpu", seed=123)
    prop_samples = trainer.rcfg.nerf.propnet.num_samples_per_prop

    # PSNR of the HIP path vs the oracle on identical rays / parameters (the second half of BASELINE.json's metric):
    # eval-mode render (no stratified jitter), composited rgb, -10 log10(mse); depth as relative error
    from emernerf_amd.render_utils import render_rays as hip_render_rays
    mods = [trainer.model, trainer.estimator] + list(trainer.props)
    for m in mods:
        m.eval()
    with torch.no_grad():
        dev_data = {k: v.to(trainer.device) for k, v in data.items()}
        hip = hip_render_rays(radiance_field=trainer.model, proposal_estimator=trainer.estimator, proposal_networks=trainer.props,
                              data_dict=dev_data, cfg=trainer.rcfg, proposal_requires_grad=False)
        orc = ref.render_rays(data, samples, prop_samples, jitters=None, training=False)
    for m in mods:
        m.train()
    mse = float(((hip["rgb"].cpu().double() - orc["rgb"].double()) ** 2).mean())
    psnr = float("inf") if mse == 0.0 else -10.0 * math.log10(mse)
    depth_rel = float(((hip["depth"].cpu().double() - orc["depth"].double()).abs() / orc["depth"].double().abs().clamp_min(1e-6)).max())
    # The timed sample IS a K-step training job on rays coloured by a synthetic ground-truth field, run by the oracle and by the
    # HIP path from identical parameters with replayed jitter (oracle/train_parity.py; tests/test_train_parity_gpu.py holds the
    # assertions): 2 warm-up + `steps` timed oracle steps, 1 step in 6 training the proposal nets, then the PSNR of an evaluation
    # render of each against the ground truth -- the second half of BASELINE.json's metric ("PSNR vs ref" after K steps).
    K = steps + 2
    co = cotrain(trainer.kind, trainer.device, K=K, rays=rays, samples=samples,
                 prop_samples=tuple(prop_samples), num_iters=200, table_init=0.3, use_graph=False, schedule_steps=1, time_oracle_from=2)
    dt = co["oracle_s_per_step"] * steps
    return {"value": rays / co["oracle_s_per_step"], "unit": "rays/s", "cores": cores, "kind": "port",
            "psnr_vs_oracle_db": min(psnr, 999.0), "depth_max_rel_err_vs_oracle": depth_rel,
            "psnr_vs_gt_after_k": {"K": K, "hip_db": co["hip_psnr_vs_gt_db"], "oracle_db": co["ref_psnr_vs_gt_db"],
                                   "loss_first_last_hip": [co["hip_losses"][0], co["hip_losses"][-1]],
                                   "loss_first_last_oracle": [co["ref_losses"][0], co["ref_losses"][-1]],
                                   "loss_max_rel_diff": co["loss_max_rel_diff"], "param_l2_diff_over_travel": co["param_l2_diff"] / co["travel"],
                                   "note": "both trained for K optimizer steps from identical parameters on rays rendered from a fixed synthetic GT "
                                           "field (second random-table model), jitter replayed; PSNR of an eval render of 2048 held-out rays vs the GT"},
            "deviation": "BASELINE.md 2.4 names configs[0] (L4 grid, 4096 x 64) for the CPU figure; this is the SAME model as the GPU line (configs[1]: "
                         f"L16/F2/T2^19 grid, full heads, proposal rounds 128 + 64) on a bounded sample of {rays} rays x {samples} samples",
            "sample": f"{steps} full optimizer steps (after 2 warm-up steps) of {rays} rays x {samples} samples (same model/config, 1 in 6 steps "
                      f"trains the proposal nets), oracle/ref_path.py on oracle/emer_oracle.c, torch {torch.get_num_threads()} "
                      f"threads + OpenMP; {dt:.1f} s"}


def source_hash() -> str:
    """sha256[:16] of the kernel sources (csrc/*.hip, *.h, include/*.h): what a recorded measurement is valid for.  The GPU
    box has no .git, so a commit id cannot be checked there; the sources of the library that ran can."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for fn in sorted(glob.glob(os.path.join(ROOT, "emernerf_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if fn.endswith((".hip", ".h")) and "_variant_" not in fn:
            h.update(os.path.basename(fn).encode())
            h.update(open(fn, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(dominant: str, D: int, F: int, args):
    """HBM bytes per launch of the dominant kernel from the newest committed rocprofv3 PMC summary
    (profiles/r*_hbm_traffic.json).  FETCH_SIZE and WRITE_SIZE need separate profiler passes of this command
    (tools/profile_round.sh), so they cannot be collected inside this process; the file name is reported next to the
    number.  Only valid for the default workload AND the kernel sources the summary was recorded on: the summary carries
    `source_sha16` (tools/profile_round.sh stamps it) and a summary of other sources gives null, with the reason."""
    import glob
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    files = sorted(glob.glob(os.path.join(root, "r*_hbm_traffic.json")))
    if not files or (args.rays, args.samples, args.kind) != (8192, 128, "static"):
        return None, None
    path = files[-1]
    try:
        j = json.load(open(path))
        if j.get("source_sha16") != source_hash():
            return None, (f"profiles/{os.path.basename(path)} was recorded on kernel sources {j.get('source_sha16')}, this run has "
                          f"{source_hash()}: not reported (re-run tools/profile_round.sh)")
        kern = {"emer_hashgrid_bwd_params_sliced": f"hashgrid_bwd_params_sliced_kernel<{D}, {F}>",
                "emer_hashgrid_fwd": f"hashgrid_fwd_kernel<{D}, {F}, float>"}[dominant]
        return j["kernels"][kern]["hbm_bytes"], (f"profiles/{os.path.basename(path)}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate "
                                                 f"passes) of this command, reads x{j['read_correction']:.2f} (gfx950 correction, calibrated); "
                                                 "recorded by tools/profile_round.sh, not in this run")
    except Exception:
        return None, None


def pmc_step_traffic(args):
    """HBM bytes of one whole step from the same PMC summary: sum over kernels of bytes per launch x launches, divided by the steps of
    the profiled command (= launches of the main table's backward, one per step).  None unless recorded on these sources."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")))
    if not files or (args.rays, args.samples, args.kind) != (8192, 128, "static"):
        return None
    try:
        j = json.load(open(files[-1]))
        if j.get("source_sha16") != source_hash():
            return None
        ks = j["kernels"]
        steps = ks["hashgrid_bwd_params_sliced_kernel<3, 2>"]["launches"]
        return {"bytes_per_step": sum(v["hbm_bytes"] * v["launches"] for v in ks.values()) / steps, "steps_profiled": steps,
                "source": f"profiles/{os.path.basename(files[-1])}"}
    except Exception:
        return None


def rccl_summary(path, world):
    """The lines of RCCL's INFO log (rank 0) that show how many ranks the communicator has and what it built."""
    keep, n = [], 0
    try:
        with open(path, errors="replace") as f:
            for line in f:
                n += 1
                if any(t in line for t in ("nranks", "nRanks", "Init COMPLETE", "Connected all", "Channel 00", "Trees", "Ring 00",
                                           "comm 0x", "via P2P", "XGMI", "xgmi", "Algo", "algo")):
                    if len(keep) < 12:
                        keep.append(line.strip()[:240])
    except OSError as e:
        return {"world_size": world, "log": f"unavailable: {e!r}"}
    return {"world_size": world, "backend": "nccl (RCCL)", "log_lines_total": n, "log_excerpt": keep}


DUMP_MAX_NUMEL = 1 << 20     # entries written per parameter tensor; larger tables are sampled
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(args, dev, world: int, batch: dict, step: int, out_dir: str, write: bool) -> None:
    """What the timed path computes, as ``out_dir/<name>.npy`` (float32), reproducibly: the timed trainer's parameters after
    init + warm-up + timed steps differ from run to run (the grid backward accumulates with float atomics, and Adam with eps 1e-15
    turns last-bit differences of near-zero gradients into steps of lr, step after step), so the last timed step is taken once more
    by a FRESH trainer -- same arguments and seed (hence the same initial parameters), same launch mode, the same batch and step
    index as the last timed step -- and its results are written: the step's return value (``loss``, ``prop_grad`` as 0 / 1), the
    gradients of the groups the step trains (``grad.model.<name>``, ``grad.prop<i>.<name>``) and every parameter of the model and
    the proposal nets after its optimizer update (``model.<name>``, ``prop<i>.<name>``).  Every rank takes the step (it contains the
    gradient exchange); rank 0 writes.  A tensor of more than DUMP_MAX_NUMEL entries is written as a fixed sample of DUMP_MAX_NUMEL
    positions (a permutation seeded by its size, sorted), so two builds of the project write the same positions."""
    import numpy as np
    from emernerf_amd.trainer import Trainer
    tr = Trainer(kind=args.kind, device=dev, num_samples=args.samples, world_size=world, table_init=args.table_init,
                 use_graph=args.graph, table_dtype=args.table_dtype)
    tr.set_step(step)
    res = tr.train_step(batch)
    torch.cuda.synchronize()
    if write:
        os.makedirs(out_dir, exist_ok=True)
        arrays = {"loss": res["loss"].detach().float().cpu().numpy(), "prop_grad": np.float32(1.0 if res["prop_grad"] else 0.0)}
        trained = [("model", tr.model)] + ([(f"prop{len(tr.props) - 1}", tr.props[-1])] if res["prop_grad"] else [])
        named = [("grad." + pre + "." + n, p.grad) for pre, m in trained for n, p in m.named_parameters()]
        named += [("model." + n, p) for n, p in tr.model.named_parameters()]
        named += [(f"prop{i}." + n, p) for i, m in enumerate(tr.props) for n, p in m.named_parameters()]
        for name, t in named:
            flat = t.detach().reshape(-1)
            if flat.numel() > DUMP_MAX_NUMEL:
                g = torch.Generator().manual_seed(flat.numel())
                idx = torch.randperm(flat.numel(), generator=g)[:DUMP_MAX_NUMEL].sort().values
                flat = flat[idx.to(flat.device)]
                name += "@sample"
            arrays[name] = flat.float().cpu().numpy()
        total = sum(np.asarray(a).nbytes for a in arrays.values())
        assert total <= DUMP_MAX_BYTES, f"--dump-outputs would write {total / 2**20:.1f} MB"
        for name, a in arrays.items():
            np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float32))
    del tr, res
    torch.cuda.empty_cache()


def measure_config(kind: str, rays: int, samples: int, dev, steps: int, warmup: int, init_steps: int, start_step: int = 1000,
                   use_graph: bool = False):
    """A short run of another BASELINE config on this GPU (rank 0, single GPU): ms/step, rays/s and the roofline of its xyzt
    encoders, with the same step definition AND the same launch mode as the headline (full optimizer step, a new seeded batch
    every step; ``use_graph``: forward + backward replayed as a captured hipGraph).  The grid kernels are bracketed by HIP events
    in an eager loop (a replay launches nothing from the host); in graph mode that is a second loop after the timed one."""
    from emernerf_amd import _lib
    from emernerf_amd.trainer import Trainer, synthetic_rays
    tr = Trainer(kind=kind, device=dev, num_samples=samples, world_size=1, use_graph=use_graph)
    tr.set_step(start_step)
    kw = dict(num_cams=3, feature_dim=64) if kind == "feature" else {}
    batches = [synthetic_rays(rays, dev, seed=3000 + i, **kw) for i in range(4)]
    for i in range(init_steps + warmup):
        tr.train_step(batches[i % 4])
    names = ["emer_hashgrid_fwd", "emer_hashgrid_fwd_jac", "emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add", "emer_hashgrid_bwd_input",
             "emer_hashgrid_bwd_input_jac"]
    timer = _lib.KernelTimer(names)
    graphed = tr.use_graph   # (False if the capture failed: Trainer falls back to eager launches with a warning)
    if not graphed:
        _lib.TIMER = timer
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.train_step(batches[i % 4])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    _lib.TIMER = None
    out = {"kind": kind, "rays": rays, "samples": samples, "steps": steps, "ms_per_step": dt * 1e3, "rays_per_s": rays / dt,
           "launch_mode": "hipGraph replay of forward+backward" if graphed else "eager"}
    if graphed:   # the event-bracketed eager loop for the grid kernels' durations (and the eager step time next to the replayed one)
        tr.use_graph = False
        for i in range(2):
            tr.train_step(batches[i % 4])
        _lib.TIMER = timer
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            tr.train_step(batches[i % 4])
        torch.cuda.synchronize()
        out["eager_ms_per_step"] = (time.perf_counter() - t0) / steps * 1e3
        _lib.TIMER = None
    us, tags = timer.elapsed_us(), timer.tags
    N = rays * samples
    dyn = tr.cfg.dynamic_xyz_encoder
    D4, L4, F4 = dyn.n_input_dims, dyn.n_levels, dyn.n_features_per_level
    def xyzt(*ks):   # launches on the xyzt grids; the evaluations whose positions need a gradient run the Jacobian-storing forward and
        return [u for k in ks for u, tg in zip(us[k], tags[k]) if tg == (D4, L4, F4)]   # the streaming input gradient [r4]
    f4 = xyzt("emer_hashgrid_fwd", "emer_hashgrid_fwd_jac")
    b4 = xyzt("emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add")   # (_add: a table's second evaluation in the step)
    i4 = xyzt("emer_hashgrid_bwd_input", "emer_hashgrid_bwd_input_jac")
    if f4 and b4:
        fb4, bb4 = grid_alg_bytes(D4, L4, F4)
        # samples per launch differ once evaluations are batched: bytes are counted per SAMPLE EVALUATION of the step
        evals = {"dynamic": 1, "flow": 6, "feature": 6}[kind]   # xyzt evaluations per sample: current (+ both warps), dynamic and flow grids
        out["roofline_xyzt"] = {
            "grid": f"D{D4}/L{L4}/F{F4}/T2^{dyn.log2_hashmap_size}", "bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "launches_per_step": {"fwd": len(f4) / steps, "bwd": len(b4) / steps, "bwd_input": len(i4) / steps},
            "ms_per_step": {"fwd": sum(f4) / 1e3 / steps, "bwd": sum(b4) / 1e3 / steps, "bwd_input": sum(i4) / 1e3 / steps},
            "sample_evaluations_per_step": evals * N, "algorithmic_bytes_per_sample": {"fwd": fb4, "bwd": bb4},
            "frac_fwd": fb4 * evals * N / (sum(f4) * 1e-6 / steps) / 1e9 / HBM_PEAK_GBPS,
            # [r6] the evaluations whose positions need a gradient also STORE d out / d x (F * D * 4 bytes per sample and level): flow
            # configs differentiate 2 N rows of the 3 N-row dynamic evaluation and the 2 N rows of the flow table at the warped points
            "frac_fwd_incl_jacobian": (fb4 * evals * N + (4 * N * L4 * F4 * D4 * 4 if kind in ("flow", "feature") and i4 else 0))
            / (sum(f4) * 1e-6 / steps) / 1e9 / HBM_PEAK_GBPS,
            "frac_bwd": bb4 * evals * N / (sum(b4) * 1e-6 / steps) / 1e9 / HBM_PEAK_GBPS}
    # [r6] the static table these configs run (default_config.yaml:62-69: D3/L10/F4/T2^20), priced like the headline's main grid
    c3 = tr.cfg.xyz_encoder
    rs = grid_roofline(timer, (c3.n_input_dims, c3.n_levels, c3.n_features_per_level), steps)
    if rs is not None:
        rs["grid"] += f"/T2^{c3.log2_hashmap_size} (static xyz table of this config)"
        out["roofline_static_grid"] = rs
    del tr
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--kind", default="static", choices=["static", "dynamic", "flow", "feature"])
    ap.add_argument("--table-init", type=float, default=None, help="U(-a,a) tables instead of tcnn's +-1e-4 init")
    ap.add_argument("--start-step", type=int, default=1000, help="training step the run starts at (1000 = steady-state "
                    "proposal schedule: 1 step in 6 trains the proposal nets, nerfacc_prop_net.py:280-296)")
    ap.add_argument("--cpu-rays", type=int, default=1024)
    ap.add_argument("--init-steps", type=int, default=48, help="untimed set-up steps before the warm-up (allocator, clocks)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the lidar-step and eval-render measurements")
    ap.add_argument("--no-second-state", action="store_true", help="skip the trained-like (table_init 0.3) roofline pass")
    ap.add_argument("--graph", action="store_true", help="(default at N = 1) replay the forward+backward of a step as a captured hipGraph")
    ap.add_argument("--eager", action="store_true", help="launch every kernel of the timed steps from Python (the default at N > 1, where "
                    "the gradient buckets are launched from inside the backward)")
    ap.add_argument("--table-dtype", default="f32", choices=["f32", "f16"], help="hash-table precision: f32 (the reference's; the headline) or "
                    "f16 (tcnn half-precision tables: fp32 master cast per call, fp32 gradient accumulation; BASELINE.md 2.2)")
    ap.add_argument("--no-fp16-state", action="store_true", help="skip the short fp16-table run behind roofline_fp16_tables")
    ap.add_argument("--no-secondary", action="store_true", help="skip the short runs of BASELINE configs[2..4] (dynamic, flow, flow and feature at "
                    "the 2048-ray per-rank shard of configs[3])")
    ap.add_argument("--secondary-steps", type=int, default=0, help="timed steps of each secondary run (0: min(--steps, 12))")
    ap.add_argument("--full", action="store_true", help="after the timed region, also run every extra measurement (other launch mode, "
                    "per-kernel breakdown and rooflines, CPU baseline, lidar step and eval render, trained-like and fp16-table states, "
                    "secondary configs); a plain run prints the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computes from the seeded "
                    "parameters (loss, gradients, updated parameters; large tables as a fixed sample) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL; must be set before the HIP runtime starts
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched through torch.distributed.run (one rank per GPU)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the hot path has no CPU fallback)")
    # Test hooks (a 1-GPU box cannot run RCCL with two ranks): EMER_BENCH_SHARE_GPU=1 puts every rank on cuda:0 and
    # EMER_BENCH_BACKEND=gloo exchanges through gloo -- the same code path end to end, not a measurement.
    share_gpu = os.environ.get("EMER_BENCH_SHARE_GPU") == "1"
    backend = os.environ.get("EMER_BENCH_BACKEND", "nccl")
    dev_index = 0 if share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device(f"cuda:{dev_index}")
    # EMER_DP_FORCE=1 with one rank: the trainer takes its data-parallel path and the real RCCL collectives execute (each a copy
    # onto itself): what the exchange code costs in launches and stream hand-offs, on the only box this container reaches
    dp = world > 1 or os.environ.get("EMER_DP_FORCE") == "1"
    rccl_log = None
    if dp:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29517")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # RCCL's own account of the communicator (ranks, rings / trees, transport) goes to a per-rank file, not to stdout
        # (the JSON line must stay alone there); rank 0 quotes the relevant lines in the result
        rccl_log = f"/tmp/emer_rccl_rank{rank}_{os.getpid()}.log"
        os.environ.setdefault("NCCL_DEBUG", "INFO")
        os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH,TUNING")
        os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend=backend)

    from emernerf_amd import _build, _lib
    if rank == 0:  # one builder; the others wait (a concurrent build would write the same object files)
        _build.build()
    if world > 1:
        dist.barrier()
    from emernerf_amd.trainer import Trainer, synthetic_rays
    # Launch mode.  One step is 86 kernel launches in 3.0 ms: the host has to enqueue one every 35 us, and boxes of this pool
    # differ (the same library: 3.02 ms on most, 3.58 ms on one with a slow host).  At N = 1 the forward + backward are
    # therefore replayed as a captured hipGraph (tested equal to eager launches); the exchange and Adam stay eager.
    args.graph = (args.graph or not dp) and not args.eager

    trainer = Trainer(kind=args.kind, device=dev, num_samples=args.samples, world_size=world, table_init=args.table_init,
                      use_graph=args.graph, table_dtype=args.table_dtype)
    trainer.set_step(args.start_step)   # (also replays the proposal schedule to its state at start_step)
    # each rank its own rays (weak scaling), and a NEW batch every step: N_BATCHES seeded batches resident in HBM, rotated
    feat_kw = dict(num_cams=3, feature_dim=64) if args.kind == "feature" else {}
    batches = [synthetic_rays(args.rays, dev, seed=1000 + 64 * rank + i, **feat_kw) for i in range(N_BATCHES)]
    it = {"i": 0}

    def next_batch():
        b = batches[it["i"] % N_BATCHES]
        it["i"] += 1
        return b

    # Setup, before the W warm-up steps the contract asks for: a fixed number of extra untimed steps (reported as
    # config.init_steps) so that the caching allocator has seen both step types (with / without proposal-net training)
    # and the GPU clocks have ramped -- otherwise a short --warmup measures start-up effects (the first ~50 steps run
    # ~15 % slower), not the step.
    for _ in range(args.init_steps):
        trainer.train_step(next_batch())
    for _ in range(args.warmup):
        trainer.train_step(next_batch())

    # HIP events inside the timed region only around the roofline kernels (the grid encode + its backward: five
    # launches per step).  Timing every entry point costs ~1.4 ms/step in event records, so the full per-kernel
    # breakdown comes from a second, separately instrumented pass after the timed region.
    grid_names = ["emer_hashgrid_fwd", "emer_hashgrid_fwd_jac", "emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add", "emer_hashgrid_bwd_params_sliced_levels",
                  "emer_hashgrid_bwd_params", "emer_hashgrid_bwd_input_jac"]
    all_names = grid_names + ["emer_hashgrid_bwd_input", "emer_linear_fwd", "emer_linear_bwd", "emer_layout_transpose",
                              "emer_render_weights_fwd", "emer_render_weights_bwd", "emer_accumulate_fwd", "emer_accumulate_bwd",
                              "emer_importance_sample", "emer_ray_points", "emer_adam_step", "emer_dir_encode", "emer_contract_fwd",
                              "emer_mlp_chain", "emer_wgrad_segmented", "emer_neck_fwd", "emer_neck_bwd", "emer_neck_bwd_fused", "emer_rgb_head_fwd", "emer_rgb_head_bwd", "emer_rgb_head_bwd_fused", "emer_rgb_head_bwd_recompute",
                              "emer_rmlp_fwd", "emer_rmlp_bwd", "emer_contract_bwd", "emer_blend_accumulate_fwd", "emer_blend_accumulate_bwd",
                              "emer_prop_loss", "emer_ray_epilogue_fwd", "emer_ray_epilogue_bwd", "emer_pixel_loss_fwd", "emer_pixel_loss_bwd",
                              "emer_trunc_exp_fwd", "emer_trunc_exp_bwd", "emer_ray_inputs_fwd", "emer_embed_grad", "emer_ray_pre_fwd",
                              "emer_ray_pre_bwd", "emer_ray_head_fwd", "emer_ray_head_bwd", "emer_ray_wgrad", "emer_lidar_loss", "emer_field_fwd",
                              "emer_density_bwd_fused", "emer_rmlp_bwd_fused", "emer_composite_rgb_fwd", "emer_composite_rgb_bwd", "emer_reg_losses_fwd6",
                              "emer_reg_losses_bwd6", "emer_aggregate3_density_fwd", "emer_aggregate3_density_bwd", "emer_flow_warp_fwd", "emer_flow_warp_bwd"]
    # (graph replay launches no kernel from Python, so there is nothing to bracket inside the timed region: with --graph
    # the roofline kernels are timed in the eager instrumented pass below instead; without --full there is no roofline)
    timer = _lib.KernelTimer(grid_names) if (rank == 0 and not args.graph and args.full) else None
    _lib.TIMER = timer

    if dp:
        dist.barrier()
        if rank == 0:
            trainer.comm_events = []   # HIP events around the exposed part of every step's gradient exchange
    # [r6] SURVEY 8(d) asks for the MEDIAN of hipEvent-timed steps: one event per step boundary on the stream the step runs on (the
    # replayed graph, the exchange and Adam all go through torch's current stream), read after the timed region.  `value` stays the
    # contract's wall-clock figure (K steps between two synchronisations, MAX over ranks); the median / p10 / p90 sit next to it.
    step_events = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i_ in range(args.steps):
        step_events[i_].record()
        trainer.train_step(next_batch())
    step_events[args.steps].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    _lib.TIMER = None
    step_ms = sorted(step_events[i_].elapsed_time(step_events[i_ + 1]) for i_ in range(args.steps))
    exposed_comm = None
    if dp and rank == 0 and trainer.comm_events:
        ev = [a.elapsed_time(b) for a, b in trainer.comm_events]
        exposed_comm = {"exposed_comm_ms": sum(ev) / len(ev), "max_ms": max(ev), "steps": len(ev), "dp_mode": trainer.dp_mode,
                        "note": "device time between the end of the backward and the optimizer step: the late (table) bucket plus the waits "
                                "for the early buckets (allreduce mode), or the reduce-scatter (rs_ag; its all-gather follows Adam and is "
                                "inside ms_per_step only)"}
    trainer.comm_events = None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs:   # the last timed step once more, from the seeded parameters (dump_outputs)
        dump_outputs(args, dev, world, batches[(it["i"] - 1) % N_BATCHES], trainer.step_count - 1, args.dump_outputs, rank == 0)

    # the other launch mode over the same number of steps, so that the line shows both.  N > 1: every rank takes these steps (they
    # contain the collectives); a replayed step exchanges its gradients after the replay (one all-reduce of the main range, nothing
    # hidden), an eager step launches the hidden buckets from inside the backward -- which of the two wins at N ranks is what this
    # second figure is for.  Same bracket as the timed region: barrier + synchronize on both sides, MAX over ranks.
    other_mode = None
    if args.full:
        was = trainer.use_graph
        trainer.use_graph = not was
        for _ in range(min(args.warmup, 6) + (8 if not was else 2)):   # (a first graph replay captures: warm it up)
            trainer.train_step(next_batch())
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        if was and rank == 0:  # the eager loop is where the roofline kernels can be bracketed: same events as an eager timed region
            timer = _lib.KernelTimer(grid_names)
            _lib.TIMER = timer
        t_o = time.perf_counter()
        for _ in range(args.steps):
            trainer.train_step(next_batch())
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt_o = time.perf_counter() - t_o
        _lib.TIMER = None
        if world > 1:
            t = torch.tensor([dt_o], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt_o = float(t.item())
        other_mode = {"mode": "hipGraph replay of forward+backward" if trainer.use_graph else "eager",
                      "ms_per_step": dt_o / args.steps * 1e3, "rays_per_s": world * args.rays * args.steps / dt_o}
        if not trainer.use_graph and not was:
            other_mode["mode"] = "eager (hipGraph capture failed: see stderr)"
        trainer.use_graph = was
    # untimed: per-kernel breakdown with every entry point instrumented.  EVERY rank takes these steps (a step contains the
    # gradient collectives: rank 0 alone would wait for its peers forever); only rank 0 records events.
    breakdown, breakdown_steps = None, min(args.steps, 12)
    if args.full:
        if rank == 0:
            breakdown = _lib.KernelTimer(all_names)
            _lib.TIMER = breakdown
        graphed, trainer.use_graph = trainer.use_graph, False  # the instrumented pass launches eagerly
        for _ in range(breakdown_steps):
            trainer.train_step(next_batch())
        torch.cuda.synchronize()
        trainer.use_graph = graphed
        _lib.TIMER = None
        if rank == 0 and timer is None:
            timer = breakdown
    # CPU baseline + render parity (PSNR / depth error of the HIP path vs the oracle on the same parameters), evaluated
    # on the state the timed region left -- before the extra measurements below train the model further
    cpu_res = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            cpu_res = cpu_baseline(trainer, args.cpu_rays, args.samples)
        except Exception as e:  # the baseline is reporting only; never lose the GPU number over it
            cpu_res = {"value": None, "unit": "rays/s", "cores": os.cpu_count(), "kind": "port", "sample": f"failed: {e!r}"}
    # The other two callers of the path, measured after the timed region (they are not part of the headline metric):
    # the lidar optimizer step of a reference iteration (train_emernerf.py:747-826) and the evaluation render loop
    # (video_utils.py:50-468: eval mode, return_decomposition, 16 384-ray chunks, results copied to the host).
    extra = {}
    if args.full and rank == 0 and world == 1 and not args.no_extras:  # single-GPU measurements (the lidar step contains the collectives)
        from emernerf_amd.trainer import synthetic_lidar_rays
        lidar = [synthetic_lidar_rays(args.rays, dev, seed=2000 + i) for i in range(4)]
        for i in range(8):
            trainer.lidar_step(lidar[i % 4])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(24):
            trainer.lidar_step(lidar[i % 4])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t1) / 24
        extra["lidar_step"] = {"ms_per_step": dt * 1e3, "rays_per_s": args.rays / dt, "rays": args.rays,
                               "note": "second optimizer step of an iteration: density-only render of lidar rays, depth + "
                                       "line-of-sight losses, backward, Adam (train_emernerf.py:747-826); not in `value`"}
        from emernerf_amd.pixel_source import PixelSource
        from emernerf_amd.video_utils import render_pixels
        src = PixelSource.synthetic(dev, num_imgs=6, height=320, width=480, seed=9)
        render_pixels(trainer.rcfg, trainer.model, trainer.estimator, src, proposal_networks=trainer.props, vis_indices=[0])
        res = render_pixels(trainer.rcfg, trainer.model, trainer.estimator, src, proposal_networks=trainer.props, vis_indices=[1, 2, 3, 4])
        extra["eval_render"] = {"rays_per_s": res["render_rays_per_s"], "image": [320, 480], "images": 4, "chunk": trainer.rcfg.render.render_chunk_size,
                                "note": "render_pixels: eval mode, return_decomposition, outputs copied to host per image; not in `value`"}
        trainer.model.train(); trainer.estimator.train()
        for p_ in trainer.props:
            p_.train()
    # Second parameter state ("trained-like"): tables ~U(-0.3, 0.3) make the density vary by orders of
    # magnitude along a ray, so the proposal sampler clusters the 128 samples -- the distribution the owner-computes
    # backward is sensitive to.  Same model, same rays, grid kernels timed with HIP events over 12 steps.
    clustered = None
    if args.full and rank == 0 and args.table_init is None and not args.no_second_state:
        t2 = Trainer(kind=args.kind, device=dev, num_samples=args.samples, world_size=1, table_init=0.3)
        t2.set_step(args.start_step)
        for _ in range(18):
            t2.train_step(next_batch())
        clustered = _lib.KernelTimer(grid_names)
        _lib.TIMER = clustered
        torch.cuda.synchronize()
        t_c = time.perf_counter()
        for _ in range(12):
            t2.train_step(next_batch())
        torch.cuda.synchronize()
        clustered_ms = (time.perf_counter() - t_c) / 12 * 1e3   # eager launches with the grid kernels bracketed by events
        _lib.TIMER = None
        if world == 1:   # ... and the same state in the headline's launch mode
            t2.use_graph = args.graph
            for _ in range(8):
                t2.train_step(next_batch())
            torch.cuda.synchronize()
            t_c = time.perf_counter()
            for _ in range(12):
                t2.train_step(next_batch())
            torch.cuda.synchronize()
            clustered_ms = {"eager_instrumented": clustered_ms, "hipgraph" if t2.use_graph else "eager": (time.perf_counter() - t_c) / 12 * 1e3}
        del t2
    # BASELINE configs[1] names fp16 tables; the headline runs the reference's fp32.  A third short run with half-precision tables
    # (fp32 master cast per call, fp32 gradient accumulation) reports the grid pair of THAT mode next to it.
    fp16_state = None
    if args.full and rank == 0 and world == 1 and args.table_dtype == "f32" and args.kind == "static" and not args.no_fp16_state:
        t3 = Trainer(kind=args.kind, device=dev, num_samples=args.samples, world_size=1, table_dtype="f16")
        t3.set_step(args.start_step)
        for _ in range(18):
            t3.train_step(next_batch())
        fp16_timer = _lib.KernelTimer(grid_names)
        _lib.TIMER = fp16_timer
        torch.cuda.synchronize()
        t16 = time.perf_counter()
        for _ in range(12):
            t3.train_step(next_batch())
        torch.cuda.synchronize()
        fp16_state = {"timer": fp16_timer, "ms_per_step": (time.perf_counter() - t16) / 12 * 1e3}
        _lib.TIMER = None
        del t3
        torch.cuda.empty_cache()
    # BASELINE configs[2..3] on the same code path, short runs (parity-test configurations, reported next to the headline so
    # that the driver's line carries them): dynamic and flow at 8192 x 128, and flow at 2048 x 128 -- the per-rank shard of
    # configs[3] ("16384 rays over 8 GPUs")
    secondary = None
    if args.full and rank == 0 and world == 1 and args.kind == "static" and not args.no_secondary:
        ss = args.secondary_steps or min(args.steps, 12)
        secondary = []
        # ... and configs[4] (flow + feature head) at its 2048-ray shard
        for kind_, rays_ in (("dynamic", args.rays), ("flow", args.rays), ("flow", max(args.rays // 4, 256)), ("feature", max(args.rays // 4, 256))):
            try:
                secondary.append(measure_config(kind_, rays_, args.samples, dev, steps=ss, warmup=4, init_steps=14, use_graph=args.graph))
            except Exception as e:  # reporting only
                secondary.append({"kind": kind_, "rays": rays_, "error": repr(e)})
    if world > 1:
        dist.barrier()

    if rank == 0:
        N = args.rays * args.samples
        c = trainer.cfg.xyz_encoder
        D, L, F = c.n_input_dims, c.n_levels, c.n_features_per_level
        step_traffic = pmc_step_traffic(args)
        workloads = {
            "static": "BASELINE.json configs[1]: static-only RadianceField",
            "dynamic": "BASELINE.json configs[2] (default_dynamic.yaml): static + dynamic xyzt grid D4/L10/F4/T2^18 + shadow head",
            "flow": "BASELINE.json configs[3] (default_flow.yaml): static + dynamic + flow xyzt grids, flow-warped temporal aggregation "
                    "(8192 rays per GPU; the config names 16384 rays over 8 GPUs)",
            "feature": "BASELINE.json configs[4]: flow model + feature head (E=64) + learnable PE, 3 cameras (8192 rays per GPU)",
        }
        if args.full:   # the figures built on the passes after the timed region
            us = timer.elapsed_us()
            tags = timer.tags

            def main_grid(name):  # launches on the main (L-level, F-feature) grid only, not the proposal grids
                return [u for u, tg in zip(us[name], tags[name]) if tg == (D, L, F)]

            fwd_b, bwd_b = grid_alg_bytes(D, L, F)
            f_us, b_us = main_grid("emer_hashgrid_fwd"), main_grid("emer_hashgrid_bwd_params_sliced")
            # data-parallel eager steps run the table's backward as two level-range launches (the first range's all-reduce starts
            # between them): one backward = the sum of a pair
            lv = main_grid("emer_hashgrid_bwd_params_sliced_levels")
            b_us = b_us + [lv[i] + lv[i + 1] for i in range(0, len(lv) - 1, 2)]
            f_avg = sum(f_us) / max(len(f_us), 1)
            b_avg = sum(b_us) / max(len(b_us), 1)

            def spread(v):   # median and the 10th / 90th percentile of the per-launch durations next to the average the roofline uses
                s_ = sorted(v)
                return {"median": s_[len(s_) // 2], "p10": s_[len(s_) // 10], "p90": s_[(9 * len(s_)) // 10], "launches": len(s_)} if s_ else None
            per_kernel = {n: {"launches_per_step": len(v) / breakdown_steps, "ms_per_step": sum(v) / 1e3 / breakdown_steps,
                              "avg_us": (sum(v) / len(v)) if v else 0.0}
                          for n, v in breakdown.elapsed_us().items() if v}
            dominant = "emer_hashgrid_bwd_params_sliced" if b_avg >= f_avg else "emer_hashgrid_fwd"
            dom_us, dom_bytes = (b_avg, bwd_b * N) if dominant.endswith("sliced") else (f_avg, fwd_b * N)
            ach = dom_bytes / (dom_us * 1e-6) / 1e9 if dom_us > 0 else 0.0
            both = (fwd_b + bwd_b) * N / ((f_avg + b_avg) * 1e-6) / 1e9 if (f_avg + b_avg) > 0 else 0.0
            traffic, traffic_src = pmc_traffic(dominant, D, F, args)
            # [r6] the proposal networks' grids (L8/F1/T2^20, default_config.yaml:51-58): two forward launches per step (8192 x 128 and
            # 8192 x 64 samples on the SAME table -- the reference's late-binding lambda), backward + in-kernel add on one step in six
            pk = PROP_SHAPE
            roof_prop = grid_roofline(timer, pk, args.steps)
            if roof_prop is not None:
                roof_prop["grid"] += "/T2^20 (proposal nets; both rounds query the last one)"
                roof_prop["timed_in"] = "the same event-bracketed loop as `roofline`"
            roof2 = None
            if clustered is not None:
                us2, tg2 = clustered.elapsed_us(), clustered.tags
                f2 = [u for u, tg in zip(us2["emer_hashgrid_fwd"], tg2["emer_hashgrid_fwd"]) if tg == (D, L, F)]
                b2 = [u for u, tg in zip(us2["emer_hashgrid_bwd_params_sliced"], tg2["emer_hashgrid_bwd_params_sliced"]) if tg == (D, L, F)]
                if f2 and b2:
                    fa, ba = sum(f2) / len(f2), sum(b2) / len(b2)
                    roof2 = {"table_init": 0.3, "ms_per_step": clustered_ms, "bound": "hbm", "kernel": "emer_hashgrid_bwd_params_sliced", "avg_us": ba,
                             "achieved": bwd_b * N / (ba * 1e-6) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                             "frac": bwd_b * N / (ba * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                             "grid_encode_plus_bwd": {"fwd_avg_us": fa, "bwd_avg_us": ba,
                                                      "frac": (fwd_b + bwd_b) * N / ((fa + ba) * 1e-6) / 1e9 / HBM_PEAK_GBPS}}
            roof16 = None
            if fp16_state is not None:
                us3, tg3 = fp16_state["timer"].elapsed_us(), fp16_state["timer"].tags
                f3 = [u for u, tg in zip(us3["emer_hashgrid_fwd"], tg3["emer_hashgrid_fwd"]) if tg == (D, L, F)]
                b3 = [u for u, tg in zip(us3["emer_hashgrid_bwd_params_sliced"], tg3["emer_hashgrid_bwd_params_sliced"]) if tg == (D, L, F)]
                if f3 and b3:
                    fa3, ba3 = sum(f3) / len(f3), sum(b3) / len(b3)
                    fwd16, bwd16 = grid_alg_bytes(D, L, F, sp=2, so=4, sg=4)   # fp16 gathers, fp32 encodings and gradient accumulation
                    roof16 = {"tables": "fp16 copy of the fp32 master per call (emer_cast_f32_f16), fp32 encodings, fp32 gradient accumulation "
                                        "(owner-computes backward, never reads the table)", "bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                              "fwd_avg_us": fa3, "bwd_avg_us": ba3, "algorithmic_bytes_per_sample": {"fwd": fwd16, "bwd": bwd16},
                              "frac_encode_plus_bwd": (fwd16 + bwd16) * N / ((fa3 + ba3) * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                              "baseline_md_target_us": 711, "pair_us": fa3 + ba3, "ms_per_step": fp16_state["ms_per_step"],
                              "note": "BASELINE.md 2.3 counts 2712 B/sample for this mode (fp16 encodings: 588 + 2124); this path keeps the "
                                      "encodings fp32 (the fused heads consume fp32): 652 + 2188 B"}
            # xyzt grids of the dynamic / flow configs (dynamic and flow encoders share one shape): their own roofline block
            roof_xyzt = None
            dyn = getattr(trainer.cfg, "dynamic_xyz_encoder", None)
            if args.kind != "static" and dyn is not None:
                D4, L4, F4 = dyn.n_input_dims, dyn.n_levels, dyn.n_features_per_level
                f4 = [u for u, tg in zip(us["emer_hashgrid_fwd"], tags["emer_hashgrid_fwd"]) if tg == (D4, L4, F4)]
                b4 = [u for k4 in ("emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add") for u, tg in zip(us[k4], tags[k4]) if tg == (D4, L4, F4)]
                if f4 and b4:
                    fb4, bb4 = grid_alg_bytes(D4, L4, F4)
                    fa4, ba4 = sum(f4) / len(f4), sum(b4) / len(b4)
                    roof_xyzt = {"grid": f"D{D4}/L{L4}/F{F4}/T2^{dyn.log2_hashmap_size} (dynamic and flow encoders)", "bound": "hbm",
                                 "launches_per_step": {"fwd": len(f4) / args.steps, "bwd": len(b4) / args.steps},
                                 "fwd_avg_us": fa4, "bwd_avg_us": ba4, "algorithmic_bytes_per_sample": {"fwd": fb4, "bwd": bb4},
                                 "frac_bwd": bb4 * N / (ba4 * 1e-6) / 1e9 / HBM_PEAK_GBPS,
                                 "frac_encode_plus_bwd": (fb4 + bb4) * N / ((fa4 + ba4) * 1e-6) / 1e9 / HBM_PEAK_GBPS, "peak": HBM_PEAK_GBPS, "unit": "GB/s"}
            # Matrix-pipe rooflines of the head kernels (static configuration only: hidden 64, geo 64).  `achieved` = algorithmic
            # (fp32-equivalent) flops of one launch / its average duration in the instrumented pass; the kernels execute SIX
            # bf16 partial products per fp32 product (exact 3-term splits, csrc/mlp_fused.hip), so the bf16 pipe does 6x that, plus -- in the
            # fused backward kernels -- the transposer passes that put rows on the reduction index (3 instructions of 16 x 16 x 32 per
            # 16 x 16 operand tile = 3072 flops per row and tile).  [r4] their weight gradients run on v_mfma_f32_32x32x16_bf16 (full K);
            # `executed` = all of that, `frac` = executed / 2.5 PFLOP/s dense bf16.
            mfma = {}
            if args.kind == "static":
                k0 = L * F
                n_out = trainer.model.base_mlp[2].out_features
                dgrad_neck, wgrad_neck = 2.0 * N * (64 * 64 + 64 * k0), 2.0 * N * (64 * n_out + 64 * k0)
                # (no "emer_neck_fwd" entry: in the static step the main neck runs inside emer_field_fwd, and the emer_neck_fwd launches
                # that remain are the proposal nets' 8 -> 64 -> 1 density MLPs on exact-fp32 matrix instructions)
                flops = {"emer_neck_bwd": (dgrad_neck, 6.0),
                         "emer_neck_bwd_fused": (dgrad_neck + wgrad_neck, None),
                         "emer_rgb_head_fwd": (2.0 * N * (64 * 64 + 128 * 64 + 64 * 3), 6.0),
                         "emer_field_fwd": (2.0 * N * (k0 * 64 + 64 * 64) + 2.0 * N * (64 * 64 + 128 * 64 + 64 * 3), 6.0),  # neck + rgb head in one launch
                         "emer_rgb_head_bwd": (2.0 * N * (3 * 64 + 3 * 64 * 64), 6.0),
                         # [r4] data gradients + the weight gradients of the per-sample column blocks (dW1 [64][128], dW0 [64][64]); the transposer
                         # handles dpre1 / dpre0 only (8 tiles per 16 rows: a1 / geo are read transposed from LDS)
                         "emer_rgb_head_bwd_fused": (2.0 * N * (3 * 64 + 3 * 64 * 64) + 2.0 * N * (64 * 128 + 64 * 64), None),
                         # [r6] the same + the recomputation of a1 / a2 (3 x 64 x 64 MACs per sample); the transposer handles dpre1 / dpre0 / a1 / geo
                         "emer_rgb_head_bwd_recompute": (2.0 * N * (3 * 64 + 3 * 64 * 64) + 2.0 * N * (64 * 128 + 64 * 64) + 2.0 * N * 3 * 64 * 64, None)}
                for kn, (fl, mult) in flops.items():
                    v = [u for u in breakdown.elapsed_us().get(kn, [])]
                    if kn.startswith("emer_neck"):  # main-field launches only (the proposal nets are the short ones; in the static step the forward runs inside emer_field_fwd)
                        v = sorted(v)[-max(1, breakdown_steps):]
                    if v:
                        t = sum(v) / len(v)
                        t_row = 3.0 * 2.0 * 16 * 32        # transposer flops per row and 16 x 16 operand tile
                        if kn == "emer_rgb_head_bwd_fused":
                            ex = 6.0 * fl + t_row * 8 * N
                        elif kn == "emer_rgb_head_bwd_recompute":
                            ex = 6.0 * fl + t_row * 16 * N
                        elif kn == "emer_neck_bwd_fused":    # tiles: h1 (4), d (4), dpre0 (4), the encoding ((k0 + 15) // 16)
                            ex = 6.0 * fl + t_row * (12 + (k0 + 15) // 16) * N
                        else:
                            ex = fl * mult
                        mfma[kn] = {"avg_us": t, "achieved": fl / (t * 1e-6) / 1e12, "executed": ex / (t * 1e-6) / 1e12, "peak": BF16_MFMA_PEAK_TFLOPS,
                                    "unit": "TFLOP/s", "frac": ex / (t * 1e-6) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                                    "vs_fp32_matrix_peak": fl / (t * 1e-6) / 1e12 / FP32_MFMA_PEAK_TFLOPS}
        out = {
            "metric": "train rays/sec (8192-ray batch, 128 samples)",
            "value": world * args.rays * args.steps / elapsed,
            "unit": "rays/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_per_step_median": step_ms[len(step_ms) // 2], "ms_per_step_p10": step_ms[len(step_ms) // 10], "ms_per_step_p90": step_ms[(9 * len(step_ms)) // 10],
            "ms_per_step_note": "median / p10 / p90 of HIP events recorded at every step boundary of the timed region (rank 0); `value` and "
                                "`ms_per_step` are the wall-clock mean of the same steps (contract), "
                                f"mean / median = {elapsed / args.steps * 1e3 / step_ms[len(step_ms) // 2]:.4f}",
            "hbm_frac_step": None if step_traffic is None else
            {"bytes_per_step": step_traffic["bytes_per_step"], "achieved": step_traffic["bytes_per_step"] / (elapsed / args.steps) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
             "frac": step_traffic["bytes_per_step"] / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBPS,
             "source": step_traffic["source"] + ": sum over kernels of PMC bytes per launch x launches / profiled steps, over this run's step time"},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.table_dtype == "f32" else "f32 (fp16 hash tables)",
            "dtype_note": "fp32 parameters, activations, gradients and accumulation; the 64-wide head GEMMs evaluate each fp32 product as six "
                          "bf16 partial products of an exact three-term split (error of the order of fp32 rounding; parity tests at the "
                          "fp32 kernels' tolerances)",
            "data": "synthetic",
            "config": {"workload": f"{workloads[args.kind]}, xyz hash grid D{D}/L{L}/F{F}/T2^{c.log2_hashmap_size} "
                                   f"({'fp32 tables, the reference precision' if args.table_dtype == 'f32' else 'fp16 tables from an fp32 master, fp32 gradient accumulation'}) + base MLP {L * F}->64->64 + rgb head 113->64->[177]->64->3 "
                                   f"+ sky head, 2 proposal nets (L8/F1/T2^20), {args.rays} rays x {args.samples} samples per GPU, "
                                   "proposal rounds 128+64, full optimizer step (Adam)",
                       "kind": args.kind, "rays_per_gpu": args.rays, "samples": args.samples,
                       "global_rays": world * args.rays, "parallelism": f"dp{world}", "dp_mode": trainer.dp_mode, "start_step": args.start_step,
                       "init_steps": args.init_steps, "ray_batches_rotated": N_BATCHES,
                       "table_init": args.table_init if args.table_init is not None else "tcnn +-1e-4", "table_dtype": args.table_dtype,
                       "launch_mode": "hipGraph replay of forward+backward (exchange + Adam eager)" if args.graph else "eager",
                       "other_launch_mode": other_mode},
            "source_sha16": source_hash(),
        }
        if args.full:
            out.update({
                "roofline": {"bound": "hbm", "kernel": dominant, "achieved": ach, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                             "frac": ach / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": traffic_src, "avg_us": dom_us, "algorithmic_bytes_per_launch": dom_bytes,
                             "timed_in": (f"HIP events on the dispatch packets of the eager loop of {args.steps} steps that follows the hipGraph-timed "
                                          "region (config.other_launch_mode; a graph replay launches nothing from the host to bracket)")
                             if (args.graph and world == 1) else "HIP events on the dispatch packets inside the timed region",
                             "grid_encode_plus_bwd": {"achieved": both, "frac": both / HBM_PEAK_GBPS, "fwd_avg_us": f_avg, "fwd_us_spread": spread(f_us), "bwd_us_spread": spread(b_us),
                                                      "bwd_avg_us": b_avg, "algorithmic_bytes": (fwd_b + bwd_b) * N}},
                "roofline_prop": roof_prop,
                "roofline_trained_like": roof2,
                "roofline_fp16_tables": roof16,
                "roofline_xyzt": roof_xyzt,
                "lidar_step": extra.get("lidar_step"),
                "eval_render": extra.get("eval_render"),
                "roofline_mfma": mfma,
                "secondary": secondary,
                "kernels": per_kernel,
                "kernels_note": f"per-kernel breakdown from a separate fully instrumented pass of {breakdown_steps} steps after the "
                                "timed region; the roofline kernels are timed with HIP events inside the timed region itself",
            })
        if dp:
            out["rccl"] = rccl_summary(os.environ.get("NCCL_DEBUG_FILE", rccl_log), world)
            out["rccl"].update({"env": {k: os.environ[k] for k in ("NCCL_ALGO", "NCCL_PROTO", "EMER_DP_MODE", "NCCL_MIN_NCHANNELS") if k in os.environ}})
            out["gradient_exchange"] = exposed_comm
        if cpu_res is not None:
            out["cpu_baseline"] = cpu_res
        import ctypes
        ctypes.CDLL(None).fflush(None)   # RCCL's version banner sits in the C stdio buffer: out now, so that the JSON line is the last line
        print(json.dumps(out), flush=True)
    if dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
