"""Every route of the route table of emernerf_amd/radiance_field.py (its module docstring) on the GPU: one forward and one backward per
case of tests/_field_routes.py, at 5 rays x 8 (or 16) samples.  Checked: the route record the forward left in ``last_routes``, the names
passed to ``_lib.call`` during each pass, and that every gradient that arrived at a parameter is finite.

tests/golden/field_routes_calls.json was recorded with tools/field_digests.py --launches --tree on the commit BEFORE the routes were
decided in one place (profiles/field_routes_ab.json), not taken from the code under test: the rewrite must launch what its parent launched."""
import json
import os

import pytest
import torch

from tests import _field_routes as T

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field_routes_calls.json")) as _f:
    EXPECTED = json.load(_f)   # case: {"forward": [...], "backward": [...]}


def test_the_table_is_covered():
    assert set(EXPECTED) == set(T.CASES)
    for key, values in T.ROUTES.items():
        assert {c["routes"][key] for c in T.CASES.values() if c["routes"] is not None} == values, key


@pytest.mark.parametrize("case_id", list(T.CASES))
def test_routes_and_library_calls(hip_lib, monkeypatch, case_id):
    from emernerf_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    model, out = T.run_case(case_id, torch.device("cuda:0"), names)
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", real)
    assert model.last_routes == (T.CASES[case_id]["routes"] or {})   # (query_flow runs no forward: nothing recorded)
    cut = names.index(T.BACKWARD)
    assert names[:cut] == EXPECTED[case_id]["forward"]
    assert names[cut + 1:] == EXPECTED[case_id]["backward"]
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert bool(grads) == (T.CASES[case_id].get("mode") != "eval_no_grad")
    for k, g in grads.items():
        assert bool(torch.isfinite(g).all()), k
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
