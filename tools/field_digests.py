"""SHA-256 digests of what RadianceField computes on the cases of tests/_field_routes.py (one per route of the route table in the module
docstring of emernerf_amd/radiance_field.py): every tensor of the result dictionary and the gradient of every parameter, from seeded
CPU-generated weights, tables, inputs and output gradients; with --launches the names passed to ``_lib.call`` in each pass and the ordered
device kernels of one ``torch.profiler`` run per case.  Run once per checkout and compare: a rewrite of the Python that chooses among the
entry points must leave every digest and every list as it was.

usage: python tools/field_digests.py [--tree DIR] [--launches] [--out file.json]
       python tools/field_digests.py --compare parent.json new.json [--out file.json]

--tree DIR imports emernerf_amd from another checkout (the parent commit in a git worktree, with the same library copied into its
emernerf_amd/lib); the cases are this checkout's either way.

Every case runs twice.  A tensor is digested only where the two runs of ONE tree agree bitwise; the others are listed under "unstable"
with the reason they cannot be compared between trees: the appearance embedding's gradient is one ``index_add_`` (float atomics), and a
table or weight gradient whose partial sums meet in float atomics depends on the order in which workgroups finish.  --compare checks
the digests that the FIRST file (the parent) reproduced."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _field_routes as T  # noqa: E402  (imports no emernerf_amd)
TREE = ROOT
if "--tree" in sys.argv:
    i = sys.argv.index("--tree")
    TREE = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    sys.path.insert(0, TREE)

UNSTABLE = "the two runs of this tree differ: float atomics (index_add_ of the embedding gradient, partial sums of a table or weight gradient)"


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def one_run(case_id, dev, names=None):
    model, out = T.run_case(case_id, dev, names)
    d = {"out " + k: sha(v) for k, v in out.items()}
    d.update({"grad " + k: sha(p.grad) for k, p in model.named_parameters() if p.grad is not None})
    return d, dict(getattr(model, "last_routes", None) or {})


def case_record(case_id, dev, launches):
    from emernerf_amd import _lib
    names, real = [], _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        first, routes = one_run(case_id, dev, names)
    finally:
        _lib.call = real
    second, _ = one_run(case_id, dev)
    rec = {"routes": routes, "digests": {k: v for k, v in first.items() if second.get(k) == v},
           "unstable": sorted(k for k, v in first.items() if second.get(k) != v)}
    if launches:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            T.run_case(case_id, dev)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and e.device_time_total > 0]
        kernels = [e.name for e in sorted(kernels, key=lambda e: e.time_range.start)]
        rec["calls"] = names
        rec["kernels"] = [k for k in kernels if "Memcpy" not in k and "Memset" not in k]
    return rec


def compare(parent_path, new_path):
    """Per case: the digests the parent reproduced, the call list and the kernel list, parent against new."""
    a, b = (json.load(open(p)) for p in (parent_path, new_path))
    res = {"trees": [a["tree"], b["tree"]], "unstable_reason": UNSTABLE, "cases": {}}
    for case_id, pa in a["cases"].items():
        nb = b["cases"][case_id]
        res["cases"][case_id] = {
            "routes": nb["routes"], "digests": len(pa["digests"]),
            "digests_equal": all(nb["digests"].get(k) == v for k, v in pa["digests"].items()),
            "differing": sorted(k for k, v in pa["digests"].items() if nb["digests"].get(k) != v),
            "excluded": pa["unstable"],
            "names_equal": set(pa["digests"]) | set(pa["unstable"]) == set(nb["digests"]) | set(nb["unstable"]),   # result keys, parameters
            "calls_equal": pa.get("calls") == nb.get("calls"), "kernels_equal": pa.get("kernels") == nb.get("kernels"),
            "calls": pa.get("calls"), "kernels": len(pa.get("kernels") or [])}
    for k in ("digests_equal", "names_equal", "calls_equal", "kernels_equal"):
        res[k] = all(c[k] for c in res["cases"].values())
    return res


def main():
    out_path = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out")
        out_path = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    if "--compare" in sys.argv:
        i = sys.argv.index("--compare")
        res = compare(sys.argv[i + 1], sys.argv[i + 2])
        brief = {k: res[k] for k in ("digests_equal", "names_equal", "calls_equal", "kernels_equal")}
    else:
        dev = torch.device("cuda:0")
        res = {"tree": os.path.relpath(TREE, ROOT), "unstable_reason": UNSTABLE,
               "cases": {c: case_record(c, dev, "--launches" in sys.argv) for c in T.CASES}}
        torch.cuda.synchronize()
        brief = {"tree": res["tree"], "cases": len(res["cases"]), "digests": sum(len(c["digests"]) for c in res["cases"].values()),
                 "unstable": sum(len(c["unstable"]) for c in res["cases"].values())}
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(json.dumps(brief) if out_path else text)


if __name__ == "__main__":
    main()
