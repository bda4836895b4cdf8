"""SHA-256 digests of what the forward and data-gradient entry points of csrc/mlp_fused.hip compute when called directly (tests/_head_calls.py:
emer_neck_fwd / _bwd, emer_rgb_head_fwd / _bwd, emer_field_fwd, emer_rmlp_fwd / _bwd), every optional pointer given and then each one null
in turn, and with --time the device-event medians of single kernels at the workload's shape, two builds of the library interleaved in one
process.  Sibling of tools/head_digests.py (the fused backwards through emernerf_amd.fused); run once per library and compare: a refactor
of those kernels must leave every digest as it was.

usage: python tools/head_entry_digests.py [--lib tag] [--out file.json]
       python tools/head_entry_digests.py --time isa_compare.json --ab tag [--runs 7] [--out file.json]

Shapes: 17 and 33 rows (partial last tile), 129 rows (nine tiles: one chunk of eight and one more), S = 16 with R in {1, 5} for the per-ray
kernels, R = 4097 and 524 289 rows (past the first trip of the grid-stride loops), and every (KT0, F) rung of the dispatch at 33 rows.
--time reads the kernels classed "changed" from the JSON of tools/isa_compare.py, times the in-tree library against libemernerf_<tag>.so
(`runs` runs each after two dropped warm-up pairs, the order alternating from pair to pair; a run is the median of 15 launches) and gives
a verdict per kernel: the median of the in-tree library's runs must lie inside the range of the other library's runs."""
import ctypes
import hashlib
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _libsel  # noqa: E402
from emernerf_amd import _lib  # noqa: E402
from tools.kbench import timeit  # noqa: E402
from tests import _head_calls as H  # noqa: E402

# L of a rung: the odd level count whose L * F features end inside input tile kt0 (kt0 = ceil(L F / 16))
RUNG_L = {1: (13, 29, 45, 61), 2: (7, 15, 23, 31), 4: (3, 7, 11, 15), 8: (1, 3, 5, 7)}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def shas(tensors):
    return {k: sha(v) for k, v in tensors.items() if v is not None}


def null_sets(names):
    return [()] + [(n,) for n in names]


def neck_digests(d, L, F, n_out, N, nulls=True):
    c = H.neck_case(L, F, n_out, N)
    tag = f"L{L} F{F} n_out{n_out} N{N}"
    full = H.neck_fwd(c)
    for null in null_sets(("h1",) + (("dens",) if n_out > 1 else ())) if nulls else [()]:
        d[f"neck_fwd {tag} null={null}"] = shas(full if not null else H.neck_fwd(c, null))
    for null in null_sets(() if n_out == 1 else (("d0", "ddens", "dcol0") + (("d1",) if n_out == 128 else ()))) if nulls else [()]:
        d[f"neck_bwd {tag} null={null}"] = shas(H.neck_bwd(c, full, null))


def rgb_digests(d, R, S, L=0, F=0, bwd=True):
    c = H.rgb_case(R, S, 49, L, F)
    tag = f"R{R} S{S}" + (f" L{L} F{F}" if L else "")
    for null in ((), ("a2",), ("a1", "a2")):
        if L:
            d[f"field_fwd {tag} null={null}"] = shas(H.field_fwd(c, null))
        else:
            d[f"rgb_head_fwd {tag} null={null}"] = shas(H.rgb_head_fwd(c, null))
    if bwd and not L:
        full = H.rgb_head_fwd(c)
        for with_dw2 in (True, False):
            d[f"rgb_head_bwd {tag} dw2={with_dw2}"] = shas(H.rgb_head_bwd(c, full, with_dw2))


def rmlp_digests(d, n_layers, lm, k0, n_out, N, nulls=True):
    c = H.rmlp_case(n_layers, lm, k0, n_out, N, sigmoid=n_out == 1)
    tag = f"layers{n_layers} {'lm' if lm else 'rm'} k0={k0} n_out{n_out} N{N}"
    full = H.rmlp_fwd(c)
    for null in null_sets(("h1",) + (("h2",) if n_layers == 3 else ())) if nulls else [()]:
        d[f"rmlp_fwd {tag} null={null}"] = shas(full if not null else H.rmlp_fwd(c, null))
    for null in null_sets(("dx",)) if nulls else [()]:
        d[f"rmlp_bwd {tag} null={null}"] = shas(H.rmlp_bwd(c, full, null))


def digests():
    d = {}
    for N in (17, 33, 129):
        neck_digests(d, 8, 1, 1, N)      # n_out 1, k0 <= 16: density_fwd_kernel
        neck_digests(d, 12, 2, 1, N)     # n_out 1, k0 > 16: neck_fwd_kernel<., ., 1>
        neck_digests(d, 16, 2, 64, N)
        neck_digests(d, 10, 4, 128, N)
        for n_layers in (2, 3):
            for lm, k0 in ((False, 64), (True, 40)):
                for n_out in (1, 6, 64):
                    rmlp_digests(d, n_layers, lm, k0, n_out, N)
    for R in (1, 5):
        rgb_digests(d, R, 16)
        rgb_digests(d, R, 16, 16, 2)
        rgb_digests(d, R, 16, 10, 4)
    # past the first trip of the grid-stride loops
    rgb_digests(d, 4097, 16, bwd=False)
    rgb_digests(d, 4097, 16, 16, 2)
    neck_digests(d, 4, 2, 64, 524289, nulls=False)
    neck_digests(d, 8, 1, 1, 524289, nulls=False)
    rmlp_digests(d, 2, True, 8, 6, 524289, nulls=False)
    # every rung at 33 rows
    for F, Ls in RUNG_L.items():
        for L in Ls:
            for n_out in (1, 64, 128):
                neck_digests(d, L, F, n_out, 33, nulls=False)
    for F, Ls in ((2, RUNG_L[2]), (4, RUNG_L[4])):
        for L in Ls:
            rgb_digests(d, 3, 16, L, F)
    for n_layers in (2, 3):
        for n_out in (6, 24):
            rmlp_digests(d, n_layers, False, 44, n_out, 33, nulls=False)
            for k0 in (8, 28, 44, 60):
                rmlp_digests(d, n_layers, True, k0, n_out, 33, nulls=False)
    return d


# ------------------------------------------------------------------------------------------------------------- timing
class Lib:
    """A second build of the library in this process, called like emernerf_amd._lib.call."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name, argtypes in _lib.SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.argtypes, fn.restype = argtypes, ctypes.c_int
        self.lib.emer_last_error.restype = ctypes.c_char_p

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise _lib.EmerError(f"{name} failed (rc={rc}): {self.lib.emer_last_error().decode()}")


def kernel_case(kernel):
    """A kernel instantiation as isa_compare names it -> fn(call) launching it once at the workload's shape (8192 rays x 128 samples =
    2^20 rows), or None when no entry point reaches it."""
    m = re.match(r"([a-z_0-9]+_kernel)(?:<([\d,]+)>)?$", kernel) or re.match(r"_ZN4emer\d+([a-z_0-9]+_kernel)E", kernel)
    if not m:
        return None
    name = m.group(1)
    t = [int(v) for v in m.group(2).split(",")] if m.lastindex and m.lastindex >= 2 and m.group(2) else []
    R, S = 8192, 128
    N = R * S
    level = lambda kt0, F: (16 * kt0) // F   # the rung's largest L  # noqa: E731
    if name == "rgb_fwd_kernel":
        c = H.rgb_case(R, S)
        o = H.rgb_head_fwd(c)
        return lambda call: H.rgb_head_fwd(c, call=call, o=o)
    if name == "rgb_bwd_kernel":
        c = H.rgb_case(R, S)
        full = H.rgb_head_fwd(c)
        o = H.rgb_head_bwd(c, full, False)
        return lambda call: H.rgb_head_bwd(c, full, False, call=call, o=o)
    if name in ("rgb_bwdw16_kernel", "rgb_bwdwr_kernel"):   # (with their reduction launch, which is the same code in both libraries)
        c = H.rgb_case(R, S)
        full = H.rgb_head_fwd(c)
        Kh, p = c["Kh"], H._ptr
        ws = H.buf(int(_lib.load().emer_rgb_head_bwd_fused_workspace(R, S)))
        o = dict(dgeo=H.buf(N, 64), s1=H.buf(R, 64), s0=H.buf(R, 64), dw0=H.buf(64, Kh + 64), dw1=H.buf(64, 128 + Kh), dw2=H.buf(3, 64), db2=H.buf(3))
        tail = (Kh, p(c["w0"]), p(c["w1"]), p(c["w2"]), p(o["dgeo"]), p(o["s1"]), p(o["s0"]), p(ws), p(o["dw0"]), Kh + 64, p(o["dw1"]), 128 + Kh,
                p(o["dw2"]), 64, p(o["db2"]), H._stream(c["geo"]))
        if name == "rgb_bwdw16_kernel":
            return lambda call: call("emer_rgb_head_bwd_fused", p(c["dout"]), p(full["out"]), p(full["a1"]), p(full["a2"]), p(c["geo"]), 64, R, S, *tail)
        a1 = p(full["a1"]) if t and t[0] else None   # <true>: a1 stored by the forward, <false>: recomputed too
        return lambda call: call("emer_rgb_head_bwd_recompute", p(c["dout"]), p(full["out"]), a1, p(c["geo"]), 64, p(c["rb"]), p(c["rb"][:, 64:]), 128,
                                 R, S, *tail)
    if name == "field_fwd_kernel":
        c = H.rgb_case(R, S, 49, level(t[0], t[1]), t[1])
        o = H.field_fwd(c)
        return lambda call: H.field_fwd(c, call=call, o=o)
    if name in ("neck_fwd_kernel", "neck_bwd_kernel", "neck_bwdw_kernel"):
        kt0, F, x = t
        n_out = {"neck_fwd_kernel": {1: 1, 4: 64, 8: 128}, "neck_bwd_kernel": {0: 1, 4: 64, 8: 128}, "neck_bwdw_kernel": {1: 64, 2: 128}}[name][x]
        if n_out == 1 and kt0 == 1 and name == "neck_fwd_kernel":
            return None   # k0 <= 16 with one output runs density_fwd_kernel
        c = H.neck_case(level(kt0, F), F, n_out, N)
        full = H.neck_fwd(c)
        if name == "neck_fwd_kernel":
            return lambda call: H.neck_fwd(c, call=call, o=full)
        if name == "neck_bwd_kernel":
            o = H.neck_bwd(c, full)
            return lambda call: H.neck_bwd(c, full, call=call, o=o)
        L, K0 = c["L"], c["L"] * F
        ws = H.buf(int(_lib.load().emer_neck_bwd_fused_workspace(L, F, N, n_out)))
        o = dict(denc=H.buf(L, N, F), dw0=H.buf(64, K0), db0=H.buf(64), dw1=H.buf(n_out, 64), db1=H.buf(n_out))
        p = H._ptr
        return lambda call: call("emer_neck_bwd_fused", p(c["d0"]), p(c["d1"]) if n_out == 128 else None, p(c["ddens"]), p(full["dens"]), p(c["enc"]), L, F, N,
                                 p(c["w0"]), p(c["b0"]), p(c["w1"]), n_out, p(o["denc"]), p(ws), p(o["dw0"]), K0, p(o["db0"]), p(o["dw1"]), 64, p(o["db1"]),
                                 H._stream(c["enc"]))
    if name in ("rmlp_fwd_kernel", "rmlp_bwd_kernel"):
        kt0, F, nl, nto = t
        c = H.rmlp_case(nl, F != 0, 64 if F == 0 else 16 * kt0, 6 if nto == 1 else 64, N)
        full = H.rmlp_fwd(c)
        if name == "rmlp_fwd_kernel":
            return lambda call: H.rmlp_fwd(c, call=call, o=full)
        o = H.rmlp_bwd(c, full)
        return lambda call: H.rmlp_bwd(c, full, call=call, o=o)
    return None


def timings(isa_json, tag, runs, warm=2):
    changed = [r["kernel"] for r in json.load(open(isa_json))["kernels"] if r["class"] == "changed"]
    other = Lib(os.path.join(os.path.dirname(_lib.LIB_PATH), f"libemernerf_{tag}.so"))
    res = {}
    for k in changed:
        fn = kernel_case(k)
        if fn is None:
            res[k] = {"verdict": "not reachable through an entry point: not timed"}
            continue
        new, old = [], []
        t_old = lambda: old.append(timeit(lambda: fn(other.call), iters=15, warmup=3)[0])   # noqa: E731
        t_new = lambda: new.append(timeit(lambda: fn(_lib.call), iters=15, warmup=3)[0])    # noqa: E731
        for i in range(warm + runs):   # the first `warm` pairs bring the clocks up and are dropped; the order alternates from pair to pair
            for t in ((t_old, t_new) if i % 2 == 0 else (t_new, t_old)):
                t()
        new, old = new[warm:], old[warm:]
        med = sorted(new)[len(new) // 2]
        res[k] = {f"{tag}_us": [round(v, 2) for v in old], "new_us": [round(v, 2) for v in new], f"{tag}_range_us": [round(min(old), 2), round(max(old), 2)],
                  "new_median_us": round(med, 2), "verdict": "inside" if min(old) <= med <= max(old) else ("faster" if med < min(old) else "SLOWER")}
        print(k, res[k]["verdict"], res[k][f"{tag}_range_us"], res[k]["new_median_us"], flush=True)
        del fn
        torch.cuda.empty_cache()
    return res


def main():
    argv = sys.argv[1:]
    opt = {}
    for key in ("--out", "--time", "--ab", "--runs"):
        if key in argv:
            i = argv.index(key)
            opt[key] = argv[i + 1]
            del argv[i:i + 2]
    if "--time" in opt:
        res = {"lib": _libsel.TAG, "against": opt["--ab"], "kernels": timings(opt["--time"], opt["--ab"], int(opt.get("--runs", 7)))}
    else:
        res = {"lib": _libsel.TAG, "digests": digests()}
    torch.cuda.synchronize()
    text = json.dumps(res, indent=1)
    if "--out" in opt:
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])) or ".", exist_ok=True)
        with open(opt["--out"], "w") as f:
            f.write(text + "\n")
        print(json.dumps({"lib": res["lib"], "entries": len(res.get("digests", res.get("kernels")))}))
    else:
        print(text)


if __name__ == "__main__":
    main()
