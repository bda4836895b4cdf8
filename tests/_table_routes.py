"""The cases of tests/test_table_routes_gpu.py (test helper, not a test module): every route of emernerf_amd/table_grad.py::route
through the two grid Functions, on the exact probe of tests/_grid_probe.py.  Imports no emernerf_amd: tools/grid_routes.py runs the
same cases on another checkout, whose way of holding a table's state it passes in as ``set_state``.

A case runs one, two or three evaluations of ONE probe (positions x, table p, gradients dout), so the table gradient must be 1, 2 or 3
times the oracle's -- bitwise: every term is a multiple of g = GP.g_params(D) and tests/test_table_grad_cpu.py proves
3 abs_sum / g < 2^24 for these shapes."""
import contextlib

import torch

from tests import _grid_probe as GP

D, LOG2_T = 3, 8
FEATURES = (1, 2)
COUNTS = (65, 257)          # a wave and a lane, a workgroup and a lane
SPLIT_LEVEL = 2             # of the probe grid's five levels
BACKWARD, BEFORE, SPLIT, COMPLETE = "<backward>", "<before>", "<split>", "<complete>"
NAN = float("nan")

# id: (feature counts, Function, what is set up, routes in the order the backwards run, multiple of the oracle's gradient)
#   sinks: inside fused.grad_sinks(True);  evals: evaluations in one graph;  state: the table has a state (fresh, .grad NaN-filled, both hooks)
CASES = {
    "direct": (FEATURES, "lm", dict(sinks=True), ["direct"], 1),
    "direct_split": (FEATURES, "lm", dict(sinks=True, split=True), ["direct_split"], 1),
    "direct add": (FEATURES, "lm", dict(sinks=True, evals=2), ["direct", "add"], 2),
    "direct add add": (FEATURES, "lm", dict(sinks=True, evals=3), ["direct", "add", "add"], 3),
    "temp_add": (FEATURES, "lm", dict(sinks=True, evals=2, replace_grad=True), ["direct", "temp_add"], 2),
    "sliced_autograd lm": (FEATURES, "lm", dict(), ["sliced_autograd"], 1),
    "sliced_autograd rm": (FEATURES, "rm", dict(), ["sliced_autograd"], 1),
    "atomic lm": (FEATURES, "lm", dict(unsupported=True), ["atomic"], 1),
    "atomic rm": (FEATURES, "rm", dict(unsupported=True), ["atomic"], 1),
    "atomic half": ((2,), "lm", dict(half=True, sparse=True), ["atomic"], 1),
    "odd-F half": ((1,), "lm", dict(half=True), ["sliced_autograd"], 1),     # summed in fp32, rounded to half once
}
PARAMS = [(case_id, F, n) for case_id, case in CASES.items() for F in case[0] for n in COUNTS]


def probe(oracle, F, n, sparse=False):
    meta, desc = GP._exact_grid(oracle, F, LOG2_T, D)
    x, p = GP._probe_positions(n, D), GP._probe_table(meta, GP.table_seed(D, F, LOG2_T))
    return meta, desc, x, p, GP.probe_dout(n, meta.n_levels, F, 7 * n + D, sparse=sparse)


def run_case(case_id, desc, x, p, dout, dev, ops, fused, set_state, patch, names):
    """One run of the case.  ``names``: the list a ``_lib.call`` recorder appends to; BACKWARD and the hook firings are appended to it
    here.  ``set_state(table, fresh, on_last_backward, on_complete, split)``; ``patch(obj, name, value)``: monkeypatch.setattr.
    -> dict(routes, grad: the table gradient, dx, at_hook: None or (lo, hi, what [lo, hi) of the gradient held when the split hook ran))"""
    _, fn, how, _, _ = CASES[case_id]
    L, F, n = desc.n_levels, desc.n_features, x.shape[0]
    evals = how.get("evals", 1)
    xd = x.to(dev).requires_grad_(True)
    go = (GP.level_major(dout, L, F) if fn == "lm" else dout).to(dev)
    master = p.to(dev).requires_grad_(True)
    at_hook = []
    if how.get("half"):   # an fp16 table with half gradients: the fp32 master gets them through the cast's backward
        encode = lambda: ops.hashgrid_encode_lm(xd, master.half(), desc, grad_dtype=torch.float16)
    else:
        master.grad = torch.full_like(master, NAN)   # last step's values: the first backward overwrites them or zeroes them
        split = (SPLIT_LEVEL, lambda prm, lo, hi: (names.append(SPLIT), at_hook.append((lo, hi, master.grad.view(-1)[lo:hi].clone())))) \
            if how.get("split") else None
        set_state(master, True, lambda: names.append(BEFORE), lambda prm: names.append(COMPLETE), split)
        encode = (lambda: ops.hashgrid_encode_lm(xd, master, desc)) if fn == "lm" else (lambda: ops.hashgrid_encode(xd, master, desc))
    if how.get("unsupported"):
        patch(ops, "sliced_supported", lambda d: False)
    with fused.grad_sinks(True) if how.get("sinks") else contextlib.nullcontext():
        outs = [encode() for _ in range(evals)]
        names.append(BACKWARD)
        if how.get("replace_grad"):   # the sinks were recorded with the contiguous .grad; the second backward finds another one
            outs[0].backward(go)
            wide = torch.zeros(2 * master.numel(), device=dev)
            wide[::2] = master.grad
            master.grad = wide[::2]
            assert not master.grad.is_contiguous()
            outs[1].backward(go)
            order = outs
        else:
            sum((o * go).sum() for o in outs).backward()
            order = outs[::-1]   # autograd runs the backward of the latest evaluation first
    torch.cuda.synchronize()
    return dict(routes=[getattr(o.grad_fn, "table_route", None) for o in order], grad=master.grad.detach().reshape(-1).contiguous(),
                dx=xd.grad.detach(), at_hook=at_hook[0] if at_hook else None)
