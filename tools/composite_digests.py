"""SHA-256 digests of every output and gradient of the compositing entry points (csrc/composite.hip and emer_ray_epilogue_fwd/bwd of
csrc/rayloss.hip) on seeded CPU-generated inputs, and with --time the device-event medians at the workload's shapes.  Run once per library
and compare: a refactor of those kernels must leave every digest as it was.

usage: python tools/composite_digests.py [--lib tag] [--time] [--out file.json]

The kernels can only go wrong at chunk boundaries, the tail, the carries and the four-wave / quad splits, so the shapes are those of
tests/_composite_probe.py: S in WALL_S x R in WALL_R for the scans, ACC_S x (1, 5) x C in ACC_C_DIGEST for accumulate, BLEND_S with and
without shadow, every residue of the wide forward's `s, s + 4, s += 8` loop (WIDE_S), the wide backward past the 16384-workgroup cap
(WIDE_CAP), the epilogue on sum w in {0, 1e-6f and its neighbours, 1, its upper neighbour}.  Each shape goes through `ops` (forward and
autograd backward; with and without rgb / rgb_sky / shadow) and through the C entry points directly, once with every optional pointer
given and once with each of them null: `ops` always passes all of them, so only the direct calls reach those branches.  Output buffers
start at 7.5, so a store that should not happen shows too."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _libsel  # noqa: E402
from emernerf_amd import _lib, ops  # noqa: E402
from emernerf_amd.ops import _ptr, _stream  # noqa: E402
from tools.kbench import timeit  # noqa: E402
from tests import _composite_probe as P  # noqa: E402

DEV = torch.device("cuda:0")
ACC_C_DIGEST = (None, 1, 3, 8, 9, 64, 65, 100)
WIDE_C_DIGEST = (1, 64, 65, 130)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)
    return t.requires_grad_(True) if grad else t


def buf(*shape):
    return torch.full(shape, 7.5, device=DEV, dtype=torch.float32)


def null_sets(names):
    """Nothing null, then each optional pointer null on its own."""
    return [()] + [(n,) for n in names]


def pick(tensors, null):
    return {k: (None if k in null else v) for k, v in tensors.items()}


def shas(tensors):
    return {k: sha(v) for k, v in tensors.items() if v is not None}


def rays(R, S):
    """Sorted edges in [0.1, 50], sigma = rand^3 * 2; from four rays on the first is empty and the last saturated."""
    rng = np.random.default_rng(31 * S + R)
    edges = np.sort(rng.random((R, S + 1)) * 49.9 + 0.1, 1).astype(np.float32)
    sg = (rng.random((R, S)) ** 3 * 2.0).astype(np.float32)
    if R >= 4:
        sg[0], sg[-1] = 0.0, 50.0
    n = lambda *sh: rng.standard_normal(sh).astype(np.float32)  # noqa: E731
    return dict(ts=edges[:, :-1], te=edges[:, 1:], sg=sg, dW=n(R, S), dT=n(R, S), dA=n(R, S), dC=n(R, S + 1), dS=n(R, 4), rgb=rng.random((R, S, 3)),
                sky=rng.random((R, 3)), d_out=n(R, 3), d_opa=n(R, 1), d_dep=n(R, 1))


# ------------------------------------------------------------------------------------------------------------ the scans
def scan_case(R, S):
    p = {k: dev(v) for k, v in rays(R, S).items()}
    ts, te, sg = p["ts"], p["te"], p["sg"]
    d = {}
    # through ops
    s = sg.clone().requires_grad_(True)
    w, T, a, cdfs, stats, tm, td = ops.render_weights(ts, te, s, want_t=True)
    ((w * p["dW"]).sum() + (T * p["dT"]).sum() + (a * p["dA"]).sum() + (cdfs * p["dC"]).sum() + (stats * p["dS"]).sum()).backward()
    d["ops.render_weights"] = shas(dict(weights=w, trans=T, alphas=a, cdfs=cdfs, stats=stats, t_mid=tm, t_dist=td, d_sigma=s.grad))
    for tag, with_rgb, with_sky in (("rgb+sky", True, True), ("rgb", True, False), ("geometry", False, False)):
        s = sg.clone().requires_grad_(True)
        c = p["rgb"].clone().requires_grad_(True) if with_rgb else None
        sk = p["sky"].clone().requires_grad_(True) if with_sky else None
        w, T, tm, td, opa, dep, med, out = ops.composite_rgb(ts, te, s, c, sk)
        loss = (opa * p["d_opa"]).sum() + (dep * p["d_dep"]).sum() + (w * p["dW"]).sum() + (T * p["dT"]).sum()
        if out is not None:
            loss = loss + (out * p["d_out"]).sum()
        loss.backward()
        d[f"ops.composite_rgb {tag}"] = shas(dict(weights=w, trans=T, t_mid=tm, t_dist=td, opacity=opa, depth=dep, median=med, rgb_out=out, d_sigma=s.grad,
                                                  d_rgb=None if c is None else c.grad, d_sky=None if sk is None else sk.grad))
    # the entry points themselves, each optional pointer null in turn
    for null in null_sets(("weights", "trans", "alphas", "cdfs", "ray_stats", "t_mid", "t_dist")):
        o = pick(dict(weights=buf(R, S), trans=buf(R, S), alphas=buf(R, S), cdfs=buf(R, S + 1), ray_stats=buf(R, 4), t_mid=buf(R, S), t_dist=buf(R, S)), null)
        _lib.call("emer_render_weights_fwd", _ptr(ts), _ptr(te), _ptr(sg), R, S, _ptr(o["weights"]), _ptr(o["trans"]), _ptr(o["alphas"]), _ptr(o["cdfs"]),
                  _ptr(o["ray_stats"]), _ptr(o["t_mid"]), _ptr(o["t_dist"]), _stream(sg))
        d[f"render_weights_fwd null={null}"] = shas(o)
    for null in null_sets(("d_weights", "d_trans", "d_alphas", "d_ray_stats")):
        g = pick(dict(d_weights=p["dW"], d_trans=p["dT"], d_alphas=p["dA"], d_ray_stats=p["dS"]), null)
        ds = buf(R, S)
        _lib.call("emer_render_weights_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(g["d_weights"]), _ptr(g["d_trans"]), _ptr(g["d_alphas"]),
                  _ptr(g["d_ray_stats"]), R, S, _ptr(ds), _stream(sg))
        d[f"render_weights_bwd null={null}"] = sha(ds)
    weights, stats = buf(R, S), buf(R, 4)
    for null in null_sets(("trans", "t_mid", "t_dist", "median_depth", "rgb_out", "rgb_sky")):
        o = pick(dict(weights=weights, trans=buf(R, S), t_mid=buf(R, S), t_dist=buf(R, S), ray_stats=stats, opacity=buf(R), depth=buf(R), median_depth=buf(R),
                      rgb_out=buf(R, 3)), null)
        _lib.call("emer_composite_rgb_fwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), None if "rgb_sky" in null else _ptr(p["sky"]), R, S, _ptr(o["weights"]),
                  _ptr(o["trans"]), _ptr(o["t_mid"]), _ptr(o["t_dist"]), _ptr(o["ray_stats"]), _ptr(o["opacity"]), _ptr(o["depth"]), _ptr(o["median_depth"]),
                  _ptr(o["rgb_out"]), _stream(sg))
        d[f"composite_rgb_fwd null={null}"] = shas(o)
    # (weights, stats: what the last forward left, the same for every null set)
    for null in null_sets(("rgb_sky", "d_rgb_out", "d_opacity", "d_depth", "d_weights", "d_trans", "d_rgb", "d_rgb_sky")):
        g = pick(dict(rgb_sky=p["sky"], d_rgb_out=p["d_out"], d_opacity=p["d_opa"], d_depth=p["d_dep"], d_weights=p["dW"], d_trans=p["dT"]), null)
        o = pick(dict(d_sigma=buf(R, S), d_rgb=buf(R, S, 3), d_rgb_sky=buf(R, 3)), null + (("d_rgb",) if "d_rgb_out" in null else ()))
        _lib.call("emer_composite_rgb_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), _ptr(g["rgb_sky"]), _ptr(weights), _ptr(stats), _ptr(g["d_rgb_out"]),
                  _ptr(g["d_opacity"]), _ptr(g["d_depth"]), _ptr(g["d_weights"]), _ptr(g["d_trans"]), R, S, _ptr(o["d_sigma"]), _ptr(o["d_rgb"]),
                  _ptr(o["d_rgb_sky"]), _stream(sg))
        d[f"composite_rgb_bwd null={null}"] = shas(o)
    return d


# ----------------------------------------------------------------------------------------------- accumulate and the blends
def accumulate_case(R, S, C):
    rng = np.random.default_rng(7 + 13 * S + R + (C or 0))
    w = dev(rng.random((R, S)))
    v = None if C is None else dev(rng.standard_normal((R, S, C)))
    go = dev(rng.standard_normal((R, C or 1)))
    wg, vg = w.clone().requires_grad_(True), None if v is None else v.clone().requires_grad_(True)
    out = ops.accumulate_along_rays(wg, vg)
    out.backward(go)
    d = {"ops": shas(dict(out=out, d_w=wg.grad, d_v=None if vg is None else vg.grad))}
    o = buf(R, C or 1)
    _lib.call("emer_accumulate_fwd", _ptr(w), _ptr(v), R, S, C or 1, _ptr(o), _stream(w))
    d["fwd"] = sha(o)
    for null in null_sets(("d_w",) if v is None else ("d_w", "d_v")):
        g = pick(dict(d_w=buf(R, S), d_v=None if v is None else buf(R, S, C)), null)
        _lib.call("emer_accumulate_bwd", _ptr(w), _ptr(v), _ptr(go), R, S, C or 1, _ptr(g["d_w"]), _ptr(g["d_v"]), _stream(w))
        d[f"bwd null={null}"] = shas(g)
    return d


def blend_case(R, S, with_shadow):
    q = {k: (None if v is None else dev(v)) for k, v in P.realistic_blend(R, S).items()}
    if not with_shadow:
        q["sh"] = None
    names = ("w", "sig", "ss", "sd", "rs", "rd", "sh")
    t = {k: (None if q[k] is None else q[k].clone().requires_grad_(True)) for k in names}
    acc, acs = ops.blend_accumulate(*(t[k] for k in names))
    loss = (acc * q["g_rgb"]).sum()
    if acs is not None:
        loss = loss + (acs * q["g_sh"]).sum()
    loss.backward()
    d = {"ops": shas(dict(acc=acc, acs=acs, **{"d_" + k: t[k].grad for k in names if t[k] is not None}))}
    ins = [_ptr(q[k]) for k in names]
    for null in null_sets(("acs",) if with_shadow else ()):
        o = pick(dict(acc=buf(R, 3), acs=buf(R) if with_shadow else None), null)
        _lib.call("emer_blend_accumulate_fwd", *ins, R, S, _ptr(o["acc"]), _ptr(o["acs"]), _stream(q["w"]))
        d[f"fwd null={null}"] = shas(o)
    outs = ("d_w", "d_sig", "d_ss", "d_sd", "d_rs", "d_rd") + (("d_sh",) if with_shadow else ())
    for null in null_sets(outs + ("g_rgb", "g_sh")):
        o = pick(dict(d_w=buf(R, S), d_sig=buf(R, S), d_ss=buf(R, S), d_sd=buf(R, S), d_rs=buf(R, S, 3), d_rd=buf(R, S, 3),
                      d_sh=buf(R, S) if with_shadow else None), null)
        g = pick(dict(g_rgb=q["g_rgb"], g_sh=q["g_sh"]), null)
        _lib.call("emer_blend_accumulate_bwd", *ins, _ptr(g["g_rgb"]), _ptr(g["g_sh"]), R, S, *(_ptr(o[k]) for k in ("d_w", "d_sig", "d_ss", "d_sd", "d_rs",
                                                                                                                      "d_rd", "d_sh")), _stream(q["w"]))
        d[f"bwd null={null}"] = shas(o)
    return d


def wide_case(R, S, C, direct=True):
    q = {k: dev(v) for k, v in P.realistic_blend(R, S, C).items()}
    names = ("w", "sig", "ss", "sd", "fs", "fd")
    t = {k: q[k].clone().requires_grad_(True) for k in names}
    acc = ops.blend_accumulate_wide(*(t[k] for k in names))
    acc.backward(q["g_acc"])
    d = {"ops": shas(dict(acc=acc, **{"d_" + k: t[k].grad for k in names}))}
    if not direct:
        return d
    ins = [_ptr(q[k]) for k in names]
    o = buf(R, C)
    _lib.call("emer_blend_accumulate_wide_fwd", *ins, R, S, C, _ptr(o), _stream(q["w"]))
    d["fwd"] = sha(o)
    outs = ("d_w", "d_sig", "d_ss", "d_sd", "d_fs", "d_fd")
    for null in null_sets(outs):
        g = pick(dict(d_w=buf(R, S), d_sig=buf(R, S), d_ss=buf(R, S), d_sd=buf(R, S), d_fs=buf(R, S, C), d_fd=buf(R, S, C)), null)
        _lib.call("emer_blend_accumulate_wide_bwd", *ins, _ptr(q["g_acc"]), R, S, C, *(_ptr(g[k]) for k in outs), _stream(q["w"]))
        d[f"bwd null={null}"] = shas(g)
    return d


# ------------------------------------------------------------------------------------------------------------ epilogue
def epilogue_case():
    p = {k: dev(v) for k, v in P.epilogue_probe().items()}
    R = p["stats"].shape[0]
    st, acc, sky = (p[k].clone().requires_grad_(True) for k in ("stats", "acc", "sky"))
    opa, dep, med, rgb = ops.ray_epilogue(st, acc, sky)
    ((opa * p["d_opa"]).sum() + (dep * p["d_dep"]).sum() + (rgb * p["d_out"]).sum()).backward()
    d = {"ops": shas(dict(opacity=opa, depth=dep, median=med, rgb=rgb, d_stats=st.grad, d_acc=acc.grad, d_sky=sky.grad))}
    for null in null_sets(("median", "rgb", "rgb_sky")):
        o = pick(dict(opacity=buf(R), depth=buf(R), median=buf(R), rgb=buf(R, 3)), null)
        _lib.call("emer_ray_epilogue_fwd", _ptr(p["stats"]), _ptr(p["acc"]), None if "rgb_sky" in null else _ptr(p["sky"]), R, _ptr(o["opacity"]), _ptr(o["depth"]),
                  _ptr(o["median"]), _ptr(o["rgb"]), _stream(p["stats"]))
        d[f"fwd null={null}"] = shas(o)
    for null in null_sets(("rgb_sky", "d_opacity", "d_depth", "d_rgb", "d_rgb_sky")):
        g = pick(dict(rgb_sky=p["sky"], d_opacity=p["d_opa"], d_depth=p["d_dep"], d_rgb=p["d_out"]), null)
        o = pick(dict(d_stats=buf(R, 4), d_rgb_sky=buf(R, 3)), null)
        _lib.call("emer_ray_epilogue_bwd", _ptr(p["stats"]), _ptr(g["rgb_sky"]), _ptr(g["d_opacity"]), _ptr(g["d_depth"]), _ptr(g["d_rgb"]), R, _ptr(o["d_stats"]),
                  _ptr(o["d_rgb_sky"]), _stream(p["stats"]))
        d[f"bwd null={null}"] = shas(o)
    return d


def digests():
    res = {}
    with torch.cuda.device(DEV):
        for S in P.WALL_S:
            for R in P.WALL_R:
                res[f"scan R{R} S{S}"] = scan_case(R, S)
        for S in P.ACC_S:
            for R in P.ACC_R:
                for C in ACC_C_DIGEST:
                    res[f"accumulate R{R} S{S} C{C}"] = accumulate_case(R, S, C)
        for S in P.BLEND_S:
            for R in (1, 5):
                for with_shadow in (True, False):
                    res[f"blend R{R} S{S} shadow{int(with_shadow)}"] = blend_case(R, S, with_shadow)
        for S in P.WIDE_S:
            for R in P.WIDE_R:
                for C in WIDE_C_DIGEST:
                    res[f"wide R{R} S{S} C{C}"] = wide_case(R, S, C)
        R, S, C = P.WIDE_CAP
        res[f"wide cap R{R} S{S} C{C}"] = wide_case(R, S, C, direct=False)
        res["epilogue"] = epilogue_case()
        torch.cuda.synchronize()
    return res


REP = 20


def timings(iters=200):
    """Median microseconds per call of each entry point at the workload's shape, 8192 rays x 128 samples; the wide blend at
    2048 x 128 x 64.  Device events (tools/kbench.py: timeit) around the replay of a graph of REP calls, divided by REP."""
    R, S = 8192, 128
    p = {k: dev(v) for k, v in rays(R, S).items()}
    ts, te, sg = p["ts"], p["te"], p["sg"]
    o = dict(w=buf(R, S), T=buf(R, S), a=buf(R, S), cdfs=buf(R, S + 1), stats=buf(R, 4), tm=buf(R, S), td=buf(R, S), opa=buf(R), dep=buf(R), med=buf(R),
             out=buf(R, 3), ds=buf(R, S), drgb=buf(R, S, 3), dsky=buf(R, 3), acc=buf(R, 3), dw=buf(R, S), dst=buf(R, 4))
    q = {k: (None if v is None else dev(v)) for k, v in P.realistic_blend(R, S).items()}
    bl = [_ptr(q[k]) for k in ("w", "sig", "ss", "sd", "rs", "rd", "sh")]
    bo = [buf(R, S) for _ in range(4)] + [buf(R, S, 3), buf(R, S, 3), buf(R, S)]
    RW, CW = 2048, 64
    qw = {k: dev(v) for k, v in P.realistic_blend(RW, S, CW).items()}
    wl = [_ptr(qw[k]) for k in ("w", "sig", "ss", "sd", "fs", "fd")]
    wo = [buf(RW, S) for _ in range(4)] + [buf(RW, S, CW), buf(RW, S, CW)]
    wacc, acs = buf(RW, CW), buf(R)
    c = lambda name, *a: _lib.call(name, *a, _stream(sg))  # noqa: E731  (the stream of the moment: the capture below runs on its own)
    fns = {
        "render_weights_fwd 8192x128": lambda: c("emer_render_weights_fwd", _ptr(ts), _ptr(te), _ptr(sg), R, S, _ptr(o["w"]), _ptr(o["T"]), _ptr(o["a"]),
                                                 _ptr(o["cdfs"]), _ptr(o["stats"]), _ptr(o["tm"]), _ptr(o["td"])),
        "render_weights_bwd 8192x128": lambda: c("emer_render_weights_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["dW"]), _ptr(p["dT"]), _ptr(p["dA"]),
                                                 _ptr(p["dS"]), R, S, _ptr(o["ds"])),
        "composite_rgb_fwd 8192x128": lambda: c("emer_composite_rgb_fwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), _ptr(p["sky"]), R, S, _ptr(o["w"]),
                                                _ptr(o["T"]), _ptr(o["tm"]), _ptr(o["td"]), _ptr(o["stats"]), _ptr(o["opa"]), _ptr(o["dep"]), _ptr(o["med"]),
                                                _ptr(o["out"])),
        "composite_rgb_bwd 8192x128": lambda: c("emer_composite_rgb_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(p["rgb"]), _ptr(p["sky"]), _ptr(o["w"]),
                                                _ptr(o["stats"]), _ptr(p["d_out"]), _ptr(p["d_opa"]), _ptr(p["d_dep"]), None, None, R, S, _ptr(o["ds"]),
                                                _ptr(o["drgb"]), _ptr(o["dsky"])),
        "accumulate_fwd C3 8192x128": lambda: c("emer_accumulate_fwd", _ptr(o["w"]), _ptr(p["rgb"]), R, S, 3, _ptr(o["acc"])),
        "accumulate_bwd C3 8192x128": lambda: c("emer_accumulate_bwd", _ptr(o["w"]), _ptr(p["rgb"]), _ptr(p["d_out"]), R, S, 3, _ptr(o["dw"]), _ptr(o["drgb"])),
        "ray_epilogue_fwd 8192": lambda: c("emer_ray_epilogue_fwd", _ptr(o["stats"]), _ptr(o["acc"]), _ptr(p["sky"]), R, _ptr(o["opa"]), _ptr(o["dep"]),
                                           _ptr(o["med"]), _ptr(o["out"])),
        "ray_epilogue_bwd 8192": lambda: c("emer_ray_epilogue_bwd", _ptr(o["stats"]), _ptr(p["sky"]), _ptr(p["d_opa"]), _ptr(p["d_dep"]), _ptr(p["d_out"]), R,
                                           _ptr(o["dst"]), _ptr(o["dsky"])),
        "blend_accumulate_fwd 8192x128": lambda: c("emer_blend_accumulate_fwd", *bl, R, S, _ptr(o["acc"]), _ptr(acs)),
        "blend_accumulate_bwd 8192x128": lambda: c("emer_blend_accumulate_bwd", *bl, _ptr(q["g_rgb"]), _ptr(q["g_sh"]), R, S, *(_ptr(t) for t in bo)),
        "blend_accumulate_wide_fwd 2048x128x64": lambda: c("emer_blend_accumulate_wide_fwd", *wl, RW, S, CW, _ptr(wacc)),
        "blend_accumulate_wide_bwd 2048x128x64": lambda: c("emer_blend_accumulate_wide_bwd", *wl, _ptr(qw["g_acc"]), RW, S, CW, *(_ptr(t) for t in wo)),
    }
    res = {}
    with torch.cuda.device(DEV):
        side = torch.cuda.Stream()
        for name, fn in fns.items():
            # these kernels take a few microseconds, less than a launch from Python and its event pair: REP calls are captured as one
            # graph (a plain chain on one stream) and the replay is timed, so the figure is device time per call
            fn()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(REP):
                    fn()
            res[name] = round(timeit(graph.replay, iters=iters, warmup=5)[0] / REP, 3)
            del graph
    return res


def main():
    out_path = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out")
        out_path = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    res = {"lib": _libsel.TAG, "digests": digests()}
    if "--time" in sys.argv:
        res["median_us"] = timings()
    torch.cuda.synchronize()
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    all_sha = hashlib.sha256(json.dumps(res["digests"], sort_keys=True).encode()).hexdigest()
    print(text if not out_path else json.dumps({"lib": res["lib"], "cases": len(res["digests"]), "sha_of_all": all_sha, "median_us": res.get("median_us")}))


if __name__ == "__main__":
    main()
