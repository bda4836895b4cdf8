"""What the two grid Functions of emernerf_amd/ops.py do on every route of the table gradient (emernerf_amd/table_grad.py::route): per case
of tests/_table_routes.py the names passed to _lib.call with the hook firings between them, the route each backward recorded (where the
checkout records one) and the SHA-256 of the table gradient and of the input gradient.  Run once per checkout and compare: a change of the
Python that chooses among the kernels must leave every list and every digest as it was.

usage: python tools/grid_routes.py [--tree DIR] [--out file.json]

--tree DIR imports emernerf_amd from another checkout (the parent commit in a git worktree, with its library built); the cases are this
checkout's either way, and the table's state is set through whichever API that checkout has: the TableGrad object of table_grad.py, or
the ``_emer_*`` attributes on the parameter that came before it."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _table_routes as T  # noqa: E402  (imports no emernerf_amd)
TREE = ROOT
if "--tree" in sys.argv:
    i = sys.argv.index("--tree")
    TREE = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
    sys.path.insert(0, TREE)
from emernerf_amd import _lib, fused, ops  # noqa: E402
from oracle import oracle as O  # noqa: E402  (the probe grid's layout; nothing is compared against it here)
assert os.path.abspath(_lib.__file__).startswith(TREE + os.sep), f"emernerf_amd was imported from {_lib.__file__}, not from {TREE}"
try:
    from emernerf_amd import table_grad
except ImportError:
    table_grad = None


def set_state(table, fresh, on_last_backward, on_complete, split):
    if table_grad is not None:
        state = table_grad.of(table, create=True)
        if fresh:
            state.begin_step()
        state.on_last_backward, state.on_complete, state.split = on_last_backward, on_complete, split
        return
    # the five attributes that the state object replaced: named here, and nowhere else in the repository, for checkouts that read them
    table._emer_grad_fresh, table._emer_pending_evals = fresh, 0
    table._emer_before_table_grad, table._emer_after_table_grad, table._emer_table_split = on_last_backward, on_complete, split


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def case(case_id, F, n):
    _, desc, x, p, dout = T.probe(O, F, n, sparse=bool(T.CASES[case_id][2].get("sparse")))
    names, real, undo = [], _lib.call, []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    patch(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        got = T.run_case(case_id, desc, x, p, dout, torch.device("cuda:0"), ops, fused, set_state, patch, names)
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
    res = {"calls": names, "grad": sha(got["grad"]), "dx": sha(got["dx"])}
    if got["at_hook"] is not None:
        lo, hi, at_hook = got["at_hook"]
        res["split"] = {"lo": lo, "hi": hi, "final_at_hook": bool(torch.equal(at_hook, got["grad"][lo:hi]))}
    if table_grad is not None:
        res["routes"] = got["routes"]
    return res


def main():
    out_path = None
    if "--out" in sys.argv:
        i = sys.argv.index("--out")
        out_path = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    O.build()
    res = {"tree": os.path.relpath(TREE, ROOT), "state": "TableGrad" if table_grad is not None else "attributes",
           "cases": {f"{case_id} F{F} n{n}": case(case_id, F, n) for case_id, F, n in T.PARAMS}}
    text = json.dumps(res, indent=1)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text + "\n")
    comparable = {k: {f: v for f, v in c.items() if f != "routes"} for k, c in res["cases"].items()}
    print(text if not out_path else json.dumps({"tree": res["tree"], "cases": len(res["cases"]),
                                                "sha_of_all": hashlib.sha256(json.dumps(comparable, sort_keys=True).encode()).hexdigest()}))


if __name__ == "__main__":
    main()
