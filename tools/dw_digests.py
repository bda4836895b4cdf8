"""SHA-256 digests of what the weight-gradient kernels of csrc/mlp.hip compute (linear_dw_kernel through ops.linear's backward, wgrad_seg_kernel /
wgrad_stream_kernel through fused.wgrad, and the reduction of the partials behind both) on seeded CPU-generated fp32 inputs, and with --time the
device-event medians at the metric shapes.  Run once per library and compare: a refactor of those kernels must leave every digest as it was.

usage: python tools/dw_digests.py [--lib tag] [--time] [--out file.json]

Shapes: ops.linear at those of tests/test_head_exact_gpu.py::test_linear_exact, fused.wgrad at those of tests/test_wgrad_exact_gpu.py.
dx is digested at every shape; dW and db only up to 960 rows: at most 15 row blocks, so the reduction runs as one split and every entry is one add
onto zero -- no order of float atomics to move a last bit.  Larger shapes are timed only."""
import ctypes
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _libsel  # noqa: E402
from emernerf_amd import fused, ops, _lib  # noqa: E402
from tools.kbench import timeit  # noqa: E402
from tests.test_wgrad_exact_gpu import CASES  # noqa: E402

DEV = torch.device("cuda:0")
LINEAR = [(64, 64, 1000, "relu"), (256, 64, 777, "relu"), (768, 256, 300, None), (3, 64, 129, None), (16, 40, 333, "relu")]   # n_out, k, rows, act
MAX_ROWS = 960
# int emer::launch_dw_reduce(const float *, int32_t, int64_t, int32_t, int32_t, float *, int64_t, float *, hipStream_t): no extern "C" entry
# point runs the reduction alone
REDUCE_SYM = "_ZN4emer16launch_dw_reduceEPKfiliiPflS2_P12ihipStream_t"


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def linear_case(n_out, k, rows, act):
    g = torch.Generator().manual_seed(n_out + k + rows)
    X, W, B = torch.randn(rows, k, generator=g), torch.randn(n_out, k, generator=g) / k ** 0.5, torch.randn(n_out, generator=g) * 0.1
    go = torch.randn(rows, n_out, generator=g)
    X, W, B = (t.to(DEV).requires_grad_(True) for t in (X, W, B))
    ops.linear(X, W, B, act).backward(go.to(DEV))
    d = {"dx": sha(X.grad)}
    if rows <= MAX_ROWS:
        d.update({"dW": sha(W.grad), "db": sha(B.grad)})
    return d


def wgrad_operands(rows, N, segs, col0, dst, seed, scale=1.0):
    """dpre, col0, the fused.seg list of one row of the case table (tests/test_wgrad_exact_gpu.py), K; seeded fp32 values from the CPU."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * scale).to(DEV)
    dpre, c0 = r(rows, N), (r(rows) if col0 else None)
    sg, col = [], 0
    for i, s in enumerate(segs):
        to = col if dst is None else dst[i]
        if s[0] == "rm":
            sg.append(fused.seg(r(rows, s[1]), col, s[1], dst_col=to)); w = s[1]
        elif s[0] == "view":
            sg.append(fused.seg(r(rows, s[2])[:, s[3]:s[3] + s[1]], col, s[1], dst_col=to)); w = s[1]
        elif s[0] == "ray":
            sg.append(fused.seg(r(rows // s[2], s[1]), col, s[1], row_div=s[2], dst_col=to)); w = s[1]
        else:
            sg.append(fused.seg_lm(r(s[1], rows, s[2]), col)); w = s[1] * s[2]
        col += w
    return dpre, c0, sg, col


def wgrad_case(name):
    rows, N, segs, want_bias, col0, ow, dst = CASES[name]
    dpre, c0, sg, K = wgrad_operands(rows, N, segs, col0, dst, seed=rows + N + len(name))
    out_w = None if ow is None else torch.zeros((N, ow), device=DEV)
    dw, db = fused.wgrad(dpre, sg, K, want_bias=want_bias, col0=c0, out_w=out_w)
    fused.join_side_stream()
    torch.cuda.synchronize()
    d = {"dW": sha(dw if out_w is None else out_w)}
    if want_bias:
        d["db"] = sha(db)
    return d


def digests():
    res = {f"linear {n}x{k} rows{rows} {act}": linear_case(n, k, rows, act) for n, k, rows, act in LINEAR}
    res.update({f"wgrad {name}": wgrad_case(name) for name in CASES if CASES[name][0] <= MAX_ROWS})
    return res


def timings(iters=30):
    """Median microseconds (device events): ops.linear's backward (dx, dW partials, reduction), fused.wgrad (partials, reduction; its workspace
    allocation and zero fill included on both sides) and the reduction alone."""
    res = {}
    r = lambda *s, k=1.0: (torch.randn(*s, generator=torch.Generator().manual_seed(sum(s) % 9973)) * k).to(DEV)
    for n, k, rows in ((64, 64, 1 << 20), (3, 64, 1 << 20), (768, 256, 1 << 17)):
        X, W, B = r(rows, k).requires_grad_(True), r(n, k, k=.1).requires_grad_(True), r(n, k=.1).requires_grad_(True)
        y, go = ops.linear(X, W, B, "relu" if n == 64 else None), r(rows, n)
        res[f"linear_bwd {n}x{k} rows 2^{rows.bit_length() - 1}"] = timeit(lambda: torch.autograd.grad(y, [X, W, B], go, retain_graph=True), iters=iters)[0]
        del X, y, go
    R, S = 8192, 128
    shapes = {"wgrad_seg<2,8> 64x177 [a1 | per-ray 49 | geo] 8192x128": (64, [("rm", 64), ("ray", 49, S), ("rm", 64)]),
              "wgrad_stream 64x128 [a1 | geo] 8192x128 (its reduction launch)": (64, [("rm", 64), ("rm", 64)]),
              "wgrad_seg<2,2> 128x64 [a] 8192x128": (128, [("rm", 64)])}
    for name, (N, segs) in shapes.items():
        dpre, _, sg, K = wgrad_operands(R * S, N, segs, False, None, seed=N + len(segs), scale=0.1)
        res[name] = timeit(lambda: fused.wgrad(dpre, sg, K), iters=iters)[0]
        del dpre, sg
    lib = _lib.load()
    if hasattr(lib, REDUCE_SYM):
        fn = getattr(lib, REDUCE_SYM)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                       ctypes.c_void_p, ctypes.c_void_p]
        nb, n, k = 256, 64, 128
        part, dw, db = r(nb, n * k + n), torch.zeros(n, k, device=DEV), torch.zeros(n, device=DEV)
        st = torch.cuda.current_stream().cuda_stream

        def red():
            assert fn(part.data_ptr(), nb, n * k + n, n, k, dw.data_ptr(), k, db.data_ptr(), st) == 0
        res["dw_reduce alone 256 partials of 64x128+64"] = timeit(red, iters=200, warmup=10)[0]
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
