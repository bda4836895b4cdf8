"""Every route of emernerf_amd/table_grad.py::route on the GPU, through ``ops.hashgrid_encode_lm`` and ``ops.hashgrid_encode``: the cases
of tests/_table_routes.py on the exact probe (tests/_grid_probe.py), where every table-gradient sum is exact in any order.  Checked per
case: the route each backward recorded (``out.grad_fn.table_route``), the table gradient BITWISE against the double-precision oracle
(times the number of evaluations), and the names passed to ``_lib.call`` with the hook firings between them.

EXPECTED was recorded with tools/grid_routes.py --tree on the commit BEFORE the grid Functions were rewritten around ``ctx.table_route``
(profiles/table_grad_routes_ab.json, the parent's column), not taken from the code under test: the rewrite must launch what its parent
launched, in the parent's order."""
import numpy as np
import pytest
import torch

from tests import _grid_probe as GP
from tests import _table_routes as T

pytestmark = pytest.mark.gpu

_FWD_LM, _FWD_RM = ["emer_hashgrid_fwd_jac"], ["emer_hashgrid_fwd", "emer_layout_transpose"]
_SLICED, _ADD, _LEVELS, _ATOMIC = ("emer_hashgrid_bwd_params_sliced", "emer_hashgrid_bwd_params_sliced_add", "emer_hashgrid_bwd_params_sliced_levels",
                                   "emer_hashgrid_bwd_params")
_DX_JAC, _DX = "emer_hashgrid_bwd_input_jac", "emer_hashgrid_bwd_input"
EXPECTED = {   # case: (forward, backward)
    "direct": (_FWD_LM, [T.BEFORE, _SLICED, T.COMPLETE, _DX_JAC]),
    "direct_split": (_FWD_LM, [T.BEFORE, _LEVELS, T.SPLIT, _LEVELS, T.COMPLETE, _DX_JAC]),
    "direct add": (_FWD_LM * 2, [_SLICED, _DX_JAC, T.BEFORE, _ADD, T.COMPLETE, _DX_JAC]),
    "direct add add": (_FWD_LM * 3, [_SLICED, _DX_JAC, _ADD, _DX_JAC, T.BEFORE, _ADD, T.COMPLETE, _DX_JAC]),
    "temp_add": (_FWD_LM * 2, [_SLICED, _DX_JAC, T.BEFORE, _SLICED, T.COMPLETE, _DX_JAC]),
    "sliced_autograd lm": (_FWD_LM, [T.BEFORE, _SLICED, _DX_JAC]),
    "sliced_autograd rm": (_FWD_RM, [T.BEFORE, "emer_layout_transpose", _SLICED, _DX]),
    "atomic lm": (_FWD_LM, [T.BEFORE, _ATOMIC, _DX_JAC]),
    "atomic rm": (_FWD_RM, [T.BEFORE, "emer_layout_transpose", _ATOMIC, _DX]),
    "atomic half": (["emer_hashgrid_fwd"], [_ATOMIC, _DX]),
    "odd-F half": (["emer_hashgrid_fwd"], [_SLICED, _DX]),
}
_REF = {}


def _reference(oracle, F, n, sparse):
    """(inputs, the oracle's table gradient), computed once per shape and shared"""
    key = (F, n, sparse)
    if key not in _REF:
        meta, desc, x, p, dout = T.probe(oracle, F, n, sparse)
        ref = oracle.hashgrid_bwd_params_bound(meta, x, dout)[0]
        ref.setflags(write=False)
        _REF[key] = (desc, x, p, dout, ref)
    return _REF[key]


def _set_state(table, fresh, on_last_backward, on_complete, split):
    from emernerf_amd import table_grad
    state = table_grad.of(table, create=True)
    if fresh:
        state.begin_step()
    state.on_last_backward, state.on_complete, state.split = on_last_backward, on_complete, split


def test_the_table_is_covered():
    from emernerf_amd import table_grad
    assert set(EXPECTED) == set(T.CASES)
    assert {r for case in T.CASES.values() for r in case[3]} == set(table_grad.ROUTES)
    assert {case[1] for case in T.CASES.values() if case[3] == ["atomic"] and not case[2].get("half")} == {"lm", "rm"}


@pytest.mark.parametrize("case_id,F,n", T.PARAMS)
def test_route_gradient_and_library_calls(hip_lib, oracle, monkeypatch, case_id, F, n):
    from emernerf_amd import _lib, fused, ops
    _, _, how, routes, times = T.CASES[case_id]
    if how.get("sparse"):
        assert n in GP.HALF_COUNTS
    desc, x, p, dout, ref = _reference(oracle, F, n, bool(how.get("sparse")))
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = T.run_case(case_id, desc, x, p, dout, torch.device("cuda:0"), ops, fused, _set_state, monkeypatch.setattr, names)
    monkeypatch.setattr(_lib, "call", real)
    assert got["routes"] == routes
    want = float(times) * ref
    if case_id == "odd-F half":
        want = want.astype(np.float16).astype(np.float64)
    GP.assert_bits(got["grad"], want, f"{case_id} F={F} n={n}: table gradient")
    cut = names.index(T.BACKWARD)
    assert (names[:cut], names[cut + 1:]) == EXPECTED[case_id]
    assert bool(torch.isfinite(got["dx"]).all())
    if how.get("split"):
        lo, hi, at_hook = got["at_hook"]
        assert (lo, hi) == (int(desc.offset[T.SPLIT_LEVEL]) * F, desc.n_entries * F)
        assert float((at_hook - got["grad"][lo:hi]).abs().max()) == 0.0, "the level range was written after its collective would have started"
