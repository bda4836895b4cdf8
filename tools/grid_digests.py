"""SHA-256 digests of what the grid kernels of csrc/hashgrid.hip compute on seeded CPU-generated inputs.  Run once per library and
compare: a refactor of those kernels must leave every digest as it was.

usage: python tools/grid_digests.py [--lib tag] [--out file.json]

Grids: tests/test_kernels_gpu.py::GRIDS.  Sample counts 1, 63, 65, 257, 1000, 4099 (a partial bitmap word, a partial workgroup, the
`n_words & 3` store path of the bitmaps); the edge rows of that module's _inputs plus one row outside [0, 1].
Digested: emer_hashgrid_fwd (fp32 / fp16 tables, level-major / row-major, with / without bitmaps: the encoding and the bitmap words without
the scratch tail), emer_hashgrid_fwd_jac at jac_row0 0 and 100, emer_hashgrid_slice_masks (which must also equal the forward's bitmaps:
exit status 1 otherwise), emer_hashgrid_bwd_input, emer_hashgrid_bwd_input_jac, and at N = 1 only -- no two lanes meet in an entry --
emer_hashgrid_bwd_params (fp32) and emer_hashgrid_bwd_params_sliced.  The table gradients at larger N are left out: atomic order and
wave scheduling move their last bits, and the per-entry bounds of the tests hold them."""
import ctypes
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import _libsel  # noqa: E402
from emernerf_amd import _lib, ops  # noqa: E402
from tests.test_kernels_gpu import GRIDS, _inputs  # noqa: E402

DEV = torch.device("cuda:0")
COUNTS = (1, 63, 65, 257, 1000, 4099)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def make_desc(name):
    D, L, base, mx, T, F = GRIDS[name]
    growth = float(np.exp((np.log(mx) - np.log(base)) / (L - 1)))
    return _lib.make_grid_desc(D, L, F, T, base, growth)


def bitmap_words(desc, n):
    return ops.mask_words(desc, n) - ops.MASK_SCRATCH


def new_masks(desc, n):
    """Zeroed: rows past a level's slice count are never written."""
    return torch.zeros((ops.mask_words(desc, n),), device=DEV, dtype=torch.int64)


def forward(desc, x, p, level_major, masks, jac_row0=None):
    N, L, F, D = x.shape[0], desc.n_levels, desc.n_features, desc.n_dims
    out = torch.empty((L, N, F) if level_major else (N, L * F), device=DEV, dtype=torch.float32)
    sn, sl = (F, N * F) if level_major else (L * F, F)
    if jac_row0 is None:
        _lib.call("emer_hashgrid_fwd", ctypes.byref(desc), ops._ptr(x), ops._ptr(p), ops._dtype_tag(p), ops._ptr(out), sn, sl, ops._ptr(masks), N,
                  ops._stream(x))
        return out, None
    jac = torch.empty((L, N - jac_row0, F, D), device=DEV, dtype=torch.float32)
    _lib.call("emer_hashgrid_fwd_jac", ctypes.byref(desc), ops._ptr(x), ops._ptr(p), ops._ptr(out), sn, sl, ops._ptr(masks), ops._ptr(jac), int(jac_row0), N,
              ops._stream(x))
    return out, jac


def grid_case(name, n, problems):
    D, L, _, _, _, F = GRIDS[name]
    desc = make_desc(name)
    meta = SimpleNamespace(n_dims=D, n_params=desc.n_entries * F)
    x, p = _inputs(meta, n, 1000 + n)
    if n >= 8:
        x[6] = torch.tensor([1.3, -0.2, 0.5, 0.1][:D])   # outside [0, 1]: the index wraps
    dlm = torch.randn(L, n, F, generator=torch.Generator().manual_seed(n)).to(DEV)
    x, p32 = x.to(DEV), p.to(DEV)
    sliced = ops.sliced_supported(desc)
    nb = bitmap_words(desc, n) if sliced else 0
    d = {}
    with torch.cuda.device(DEV):
        fwd_bits = None
        for tag, p in (("f32", p32), ("f16", p32.half())):
            for lm in (True, False):
                for want in ((False, True) if sliced else (False,)):
                    masks = new_masks(desc, n) if want else None
                    out, _ = forward(desc, x, p, lm, masks)
                    key = f"fwd {tag} {'lm' if lm else 'rm'}{' masks' if want else ''}"
                    d[key] = sha(out)
                    if want:
                        d[key + " bitmaps"] = sha(masks[:nb])
                        fwd_bits = d[key + " bitmaps"] if fwd_bits is None else fwd_bits
                        if d[key + " bitmaps"] != fwd_bits:
                            problems.append(f"{name} n={n}: the bitmaps of '{key}' differ from the first forward's")
        if sliced:
            masks = new_masks(desc, n)
            _lib.call("emer_hashgrid_slice_masks", ctypes.byref(desc), ops._ptr(x), ops._ptr(masks), n, ops._stream(x))
            d["slice_masks"] = sha(masks[:nb])
            if d["slice_masks"] != fwd_bits:
                problems.append(f"{name} n={n}: emer_hashgrid_slice_masks differs from the forward's bitmaps")
        for row0 in (0, 100):
            if row0 and n <= 100:
                continue
            masks = new_masks(desc, n) if sliced else None
            out, jac = forward(desc, x, p32, True, masks, jac_row0=row0)
            d[f"fwd_jac row0={row0}"] = sha(out)
            d[f"fwd_jac row0={row0} jac"] = sha(jac)
            if sliced:
                d[f"fwd_jac row0={row0} bitmaps"] = sha(masks[:nb])
            dx = torch.empty((n - row0, D), device=DEV, dtype=torch.float32)
            _lib.call("emer_hashgrid_bwd_input_jac", ctypes.byref(desc), ops._ptr(jac), ops._ptr(dlm[:, row0:].contiguous()), F, (n - row0) * F, ops._ptr(dx),
                      n - row0, ops._stream(x))
            d[f"bwd_input_jac row0={row0}"] = sha(dx)
        for tag, p in (("f32", p32), ("f16", p32.half())):
            dx = torch.empty((n, D), device=DEV, dtype=torch.float32)
            _lib.call("emer_hashgrid_bwd_input", ctypes.byref(desc), ops._ptr(x), ops._ptr(p), ops._dtype_tag(p), ops._ptr(dlm), F, n * F, ops._ptr(dx), n,
                      ops._stream(x))
            d[f"bwd_input {tag}"] = sha(dx)
        if n == 1:
            grad = torch.zeros(desc.n_entries * F, device=DEV, dtype=torch.float32)
            _lib.call("emer_hashgrid_bwd_params", ctypes.byref(desc), ops._ptr(x), ops._ptr(dlm), F, n * F, ops._ptr(grad), ops._dtype_tag(grad), n,
                      ops._stream(x))
            d["bwd_params f32"] = sha(grad)
            if sliced:
                masks = new_masks(desc, n)
                forward(desc, x, p32, True, masks)
                grad = torch.full((desc.n_entries * F,), float("nan"), device=DEV, dtype=torch.float32)   # every entry is overwritten
                _lib.call("emer_hashgrid_bwd_params_sliced", ctypes.byref(desc), ops._ptr(x), ops._ptr(dlm), F, n * F, ops._ptr(masks), ops._ptr(grad), n,
                          ops._stream(x))
                d["bwd_params_sliced"] = sha(grad)
        torch.cuda.synchronize()
    return d


def main():
    out_path = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out")
        out_path = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    problems = []
    res = {"lib": _libsel.TAG, "digests": {f"{name} n={n}": grid_case(name, n, problems) for name in GRIDS for n in COUNTS}, "problems": problems}
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    all_sha = hashlib.sha256(json.dumps(res["digests"], sort_keys=True).encode()).hexdigest()
    print(text if not out_path else json.dumps({"lib": res["lib"], "cases": len(res["digests"]), "digests": sum(len(v) for v in res["digests"].values()),
                                                "sha_of_all": all_sha, "problems": problems}))
    sys.exit(1 if problems else 0)


if __name__ == "__main__":
    main()
