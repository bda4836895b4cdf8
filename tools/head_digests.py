"""SHA-256 digests of what the fused heads compute through emernerf_amd.fused on seeded CPU-generated inputs: the heads with
register-resident weight gradients at their probe shapes (emer_rgb_head_bwd_fused, emer_rgb_head_bwd_recompute, emer_neck_bwd_fused,
emer_rmlp_bwd_fused) and EVERY path of the path table of fused.py (tests/_fused_paths.py: the flag matrix, density_mlp, base_mlp, skip_mlp3,
the chain shapes); with --launches the library calls and the device kernels of each path, with --time the device-event medians of the
fused backwards at the metric shapes.  Run once per library or per checkout and compare: a refactor of those kernels, or of the Python
that chooses among them, must leave every digest and every list as it was.

usage: python tools/head_digests.py [--tree DIR] [--lib tag] [--launches] [--time] [--out file.json]

--tree DIR imports emernerf_amd from another checkout (the parent commit in a git worktree, with its library built); the cases are
this checkout's either way.

Digested: the outputs and data gradients at every shape; the weight and bias gradients only where their final reduction meets in no float
atomic (at most 16 rays / 128 rows: one workgroup range), as tests/test_fused_gpu.py documents for the bitwise test."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _fused_paths as T  # noqa: E402  (imports no emernerf_amd)
TREE = ROOT
if "--tree" in sys.argv:
    i = sys.argv.index("--tree")
    TREE = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    sys.path.insert(0, TREE)
from tools import _libsel  # noqa: E402
from emernerf_amd import fused, _lib  # noqa: E402
from tools.kbench import timeit  # noqa: E402

DEV = torch.device("cuda:0")
RGB = [(1, 16, 49, 64), (5, 16, 49, 128), (16, 64, 49, 64), (2, 96, 17, 192), (1031, 32, 49, 64)]   # R, S, Kh, ld
NECK = [(4, 2, 64, 16), (8, 1, 64, 33), (10, 4, 128, 777), (3, 8, 64, 100), (16, 2, 128, 1000)]      # L, F, NG, N
RMLP = [((64, 64, 1), 1000), ((40, 64, 64, 6), 777), ((43, 32, 5), 17), ((64, 64, 64, 64), 4096)]    # dims, N (row-major input)
RMLP_LM = [(10, 4, (64, 64, 6), 1000), (4, 4, (64, 64, 64), 50)]                                     # L, F, dims, N (level-major input)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def rgb_inputs(R, S, Kh, ld, seed):
    g = torch.Generator().manual_seed(seed)
    K0 = Kh + 64
    hray, feats = torch.randn(R, Kh, generator=g), torch.randn(R * S, ld, generator=g)
    Ws = [torch.randn(64, K0, generator=g) / K0 ** 0.5, torch.randn(64, generator=g) * 0.1, torch.randn(64, 64 + K0, generator=g) / (64 + K0) ** 0.5,
          torch.randn(64, generator=g) * 0.1, torch.randn(3, 64, generator=g) / 8, torch.randn(3, generator=g) * 0.1]
    go = torch.randn(R * S, 3, generator=g)
    return hray.to(DEV), feats.to(DEV), [w.to(DEV) for w in Ws], go.to(DEV)


def rgb_case(R, S, Kh, ld, mode):
    fused.RGB_RECOMPUTE = mode
    hray, feats, Ws, go = rgb_inputs(R, S, Kh, ld, R * S + Kh)
    hd, fd = hray.requires_grad_(True), feats.requires_grad_(True)
    wd = [w.requires_grad_(True) for w in Ws]
    rgb = fused.rgb_head(hd, fd[:, :64], S, *wd)
    (rgb * go).sum().backward()
    d = {"out": sha(rgb), "dhray": sha(hd.grad), "dgeo": sha(fd.grad)}
    if R <= 16:
        d.update({f"dparam{i}": sha(w.grad) for i, w in enumerate(wd)})
    return d


def neck_case(L, F, NG, N):
    g = torch.Generator().manual_seed(L * 7 + NG + N)
    K0 = L * F
    vals = [torch.randn(L, N, F, generator=g), torch.randn(64, K0, generator=g) / K0 ** 0.5, torch.randn(64, generator=g) * 0.1,
            torch.randn(NG, 64, generator=g) / 8, torch.randn(NG, generator=g) * 0.1]
    gg, gs, gd = torch.randn(N, 64, generator=g).to(DEV), torch.randn(N, 64, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
    t = [v.to(DEV).requires_grad_(True) for v in vals]
    geo, sem, dens = fused.neck(*t)
    loss = (geo * gg).sum() + (dens * gd).sum()
    if sem is not None:
        loss = loss + (sem * gs).sum()
    loss.backward()
    d = {"geo": sha(geo), "dens": sha(dens), "denc": sha(t[0].grad)}
    if sem is not None:
        d["sem"] = sha(sem)
    if N <= 128:
        d.update({f"dparam{i}": sha(v.grad) for i, v in enumerate(t[1:])})
    return d


def rmlp_case(dims, N, lm=None):
    g = torch.Generator().manual_seed(sum(dims) + N + (0 if lm is None else 100 * lm[0]))
    if lm is None:
        x, widths = torch.randn(N, dims[0], generator=g), dims
    else:
        x, widths = torch.randn(lm[0], N, lm[1], generator=g), (lm[0] * lm[1],) + dims
    Ws = [torch.randn(widths[i + 1], widths[i], generator=g) / widths[i] ** 0.5 for i in range(len(widths) - 1)]
    Bs = [torch.randn(widths[i + 1], generator=g) * 0.1 for i in range(len(widths) - 1)]
    w = torch.randn(N, widths[-1], generator=g).to(DEV)
    t = [v.to(DEV).requires_grad_(True) for v in [x] + Ws + Bs]
    n = len(Ws)
    out = (fused.seq_mlp if lm is None else fused.seq_mlp_lm)(t[0], t[1:1 + n], t[1 + n:], _lib.ACT_SIGMOID if widths[-1] == 1 else _lib.ACT_NONE)
    (out * w).sum().backward()
    d = {"out": sha(out), "dx": sha(t[0].grad)}
    if N <= 128:
        d.update({f"dparam{i}": sha(v.grad) for i, v in enumerate(t[1:])})
    return d


def path_case(case_id):
    outs, leaves = T.run_case(case_id, DEV)
    d = {f"out{i}": sha(o) for i, o in enumerate(outs)}
    rows = T.CASES[case_id][3][1]
    few = rows <= (16 if case_id.startswith("rgb") else 128)
    d.update({f"d{i}": sha(t.grad) for i, t in enumerate(leaves) if i < (2 if case_id.startswith("rgb") else 1) or few})
    return d


def digests():
    res = {}
    for R, S, Kh, ld in RGB:
        for mode in (0, 1, 2):
            res[f"rgb R{R} S{S} Kh{Kh} ld{ld} recompute{mode}"] = rgb_case(R, S, Kh, ld, mode)
    fused.RGB_RECOMPUTE = 0
    for L, F, NG, N in NECK:
        res[f"neck L{L} F{F} NG{NG} N{N}"] = neck_case(L, F, NG, N)
    for dims, N in RMLP:
        res[f"rmlp {dims} N{N}"] = rmlp_case(dims, N)
    for L, F, dims, N in RMLP_LM:
        res[f"rmlp_lm L{L} F{F} {dims} N{N}"] = rmlp_case(dims, N, lm=(L, F))
    for case_id in T.CASES:
        res["path " + case_id] = path_case(case_id)
    return res


def launches():
    """Per path: the names passed to _lib.call (forward, T.BACKWARD, backward) and the ordered device kernels of forward + backward from
    one torch.profiler run (torch's own elementwise and fill kernels included; copies and memsets are no kernels)."""
    from torch.profiler import ProfilerActivity, profile
    res = {}
    real = _lib.call
    for case_id in T.CASES:
        names = []
        _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
        try:
            T.run_case(case_id, DEV, names)
        finally:
            _lib.call = real
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            T.run_case(case_id, DEV)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.device_time_total > 0]
        kernels = [e.name for e in sorted(kernels, key=lambda e: e.time_range.start)]
        res[case_id] = {"calls": names, "kernels": [k for k in kernels if "Memcpy" not in k and "Memset" not in k]}
    return res


def timings(iters=15):
    """Median microseconds (device events) of one backward through each entry point at the metric shapes.  The backward of a head is the
    register-resident kernel plus its small reduction launches; the forward is outside the timed region."""
    res = {}
    r = lambda *s, k=1.0: (torch.randn(*s, generator=torch.Generator().manual_seed(sum(s) % 9973)) * k).to(DEV)

    def bwd_time(make_out, leaves):
        outs = make_out()
        gos = [torch.ones_like(o) for o in outs]

        def fn():
            torch.autograd.grad(outs, leaves, gos, retain_graph=True)
        return timeit(fn, iters=iters, warmup=3)[0]

    R, S, Kh = 8192, 128, 49
    hray, geo = r(R, Kh).requires_grad_(True), r(R * S, 64).requires_grad_(True)
    Pc = [v.requires_grad_(True) for v in (r(64, Kh + 64, k=.1), r(64, k=.1), r(64, 64 + Kh + 64, k=.1), r(64, k=.1), r(3, 64, k=.1), r(3, k=.1))]
    for mode, name in ((0, "rgb_head_bwd_fused 8192x128"), (1, "rgb_head_bwd_recompute a1+a2 8192x128"), (2, "rgb_head_bwd_recompute a2 8192x128")):
        fused.RGB_RECOMPUTE = mode
        res[name] = bwd_time(lambda: [fused.rgb_head(hray, geo, S, *Pc)], [hray, geo] + Pc)
    fused.RGB_RECOMPUTE = 0
    del hray, geo
    N = 1 << 20
    for L, F, NG in ((16, 2, 128), (10, 4, 64)):
        enc = r(L, N, F).requires_grad_(True)
        Pn = [v.requires_grad_(True) for v in (r(64, L * F, k=.2), r(64, k=.1), r(NG, 64, k=.1), r(NG, k=.1))]

        def mk():
            g0, sem, dens = fused.neck(enc, *Pn)
            return [g0, dens] if sem is None else [g0, sem, dens]
        res[f"neck_bwd_fused L{L} F{F} n_out{NG} 1M"] = bwd_time(mk, [enc] + Pn)
        del enc
    enc = r(10, N, 4).requires_grad_(True)
    Wf = [v.requires_grad_(True) for v in (r(64, 40, k=.2), r(64, 64, k=.1), r(6, 64, k=.1))]
    Bf = [v.requires_grad_(True) for v in (r(64, k=.1), r(64, k=.1), r(6, k=.1))]
    res["rmlp_bwd_fused flow 40-64-64-6 1M"] = bwd_time(lambda: [fused.seq_mlp_lm(enc, Wf, Bf)], [enc] + Wf + Bf)
    return res


def main():
    out_path = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out")
        out_path = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    res = {"lib": _libsel.TAG, "tree": os.path.relpath(TREE, ROOT), "digests": digests()}
    if "--launches" in sys.argv:
        res["launches"] = launches()
    if "--time" in sys.argv:
        res["median_us"] = timings()
    torch.cuda.synchronize()
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text if not out_path else json.dumps({"lib": res["lib"], "cases": len(res["digests"]), "median_us": res.get("median_us")}))


if __name__ == "__main__":
    main()
