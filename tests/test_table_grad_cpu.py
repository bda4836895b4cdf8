"""emernerf_amd/table_grad.py on the host: the route table against a transcription of the conditionals it replaced, the evaluation
count, the stale-buffer rule on CPU tensors, the inert state, and the exactness premise of tests/test_table_routes_gpu.py."""
import itertools

import pytest
import torch

from emernerf_amd import table_grad
from emernerf_amd.table_grad import TableGrad, route
from tests import _grid_probe as GP
from tests import _table_routes as T


def _parent_route(sliced, sink, has_grad, fresh, contiguous, last_and_split):
    """``_HashGridLMFn.backward`` of commit 407d9fd, emernerf_amd/ops.py:342-380, with its tensors replaced by what it asks of them:
    ``masks is not None`` (sliced, :344), ``ctx.param is not None`` (sink, recorded by the forward at :323-324), ``param.grad is not
    None`` (has_grad), the parameter's fresh mark (fresh, :346), ``param.grad.is_contiguous()`` and ``last and 0 < split[0] < L`` of the
    table's split attribute (:352-353).  ``_HashGridFn.backward`` (:232-245) is the same with no sink: temporary + autograd
    under masks (:234-238), atomics without (:239-242)."""
    if sliced:                                                                # :344
        param = sink                                                          # :345
        direct = param and fresh and has_grad                                 # :346
        add = (not direct) and param and has_grad and contiguous              # :348
        split = last_and_split if direct else False                           # :352
        if split:                                                             # :353
            launches = "two level ranges, the hook between them"              # :356-361
        else:
            launches = "sliced_add" if add else "sliced"                      # :363-364
        if direct:                                                            # :365  (grad = None: nothing returns through autograd)
            assert launches != "sliced_add"
            return "direct_split" if split else "direct"
        elif add:                                                             # :368
            assert launches == "sliced_add"
            return "add"
        elif param and has_grad:                                              # :370  (.grad.add_(temporary))
            assert launches == "sliced"
            return "temp_add"
        assert launches == "sliced"
        return "sliced_autograd"                                              # :379  (the temporary goes back through autograd)
    return "atomic"                                                           # :373-376, :379


def test_route_is_the_parents_conditionals_on_every_input():
    seen = set()
    for args in itertools.product((False, True), repeat=6):
        assert route(*args) == _parent_route(*args), args
        seen.add(route(*args))
        if not args[1]:   # no sink (the row-major Function never records one): atomics, or a temporary handed to autograd
            assert route(*args) == ("sliced_autograd" if args[0] else "atomic")
    assert seen == set(table_grad.ROUTES) == {"atomic", "sliced_autograd", "direct", "direct_split", "add", "temp_add"}


def test_route_docstring_rows():
    """the table of the docstring (and of DESIGN.md 4.1), row by row; '-' stands for both values"""
    rows = [line.split("|")[1:-1] for line in route.__doc__.splitlines() if line.strip().startswith("| ") and "sliced (masks" not in line]
    assert len(rows) == 7
    for *cells, want in ([c.strip() for c in row] for row in rows):
        for args in itertools.product(*[{"yes": (True,), "no": (False,), "-": (False, True)}[c] for c in cells]):
            assert route(*args) == want, (cells, args)


@pytest.mark.parametrize("evals", [1, 2, 3])
def test_hooks_fire_on_the_last_backward_only(evals):
    fired, done = [], []
    s = TableGrad()
    s.on_last_backward = lambda: fired.append(len(fired))
    s.on_complete = done.append
    s.begin_step()
    s.count_eval()                      # a forward without a backward (an eval render between steps) ...
    s.begin_step()                      # ... does not shift the next step's count
    for _ in range(evals):
        s.count_eval()
    assert s.pending_evals == evals
    last = [s.enter_backward() for _ in range(evals)]
    assert last == [False] * (evals - 1) + [True] and fired == [0] and s.pending_evals == 0
    for is_last, in_place in itertools.product((False, True), repeat=2):
        s.complete("p", is_last, in_place)
    assert done == ["p"], "on_complete fires only for last and in_place"


def test_nothing_is_counted_without_a_hook():
    s = TableGrad()
    s.begin_step()
    s.count_eval()
    assert s.pending_evals == 0 and s.enter_backward() is False and s.pending_evals == 0
    s.complete("p", True, True)
    s.on_complete = lambda p: None      # either hook switches the count on
    s.count_eval()
    assert s.pending_evals == 1 and s.enter_backward() is True


def test_stale_rule_on_cpu_tensors():
    p = torch.nn.Parameter(torch.zeros(6))
    p.grad = torch.full((6,), 7.0)      # last step's values
    s = table_grad.of(p, create=True)
    assert table_grad.of(p) is s and s.fresh is False
    s.returning_through_autograd(p)
    assert bool((p.grad == 7.0).all()), "not fresh: AccumulateGrad adds onto this step's earlier gradient"
    s.begin_step()
    s.returning_through_autograd(p)
    assert s.fresh is False and not p.grad.any()
    p.grad += 3.0                       # (AccumulateGrad's add)
    s.returning_through_autograd(p)     # a second gradient of the same step: nothing is zeroed again
    assert bool((p.grad == 3.0).all())
    # finish_grads: a table that no backward wrote is zeroed, one that was written is left
    s.begin_step()
    assert s.take_stale(p.grad) is True and not p.grad.any() and s.fresh is False
    p.grad += 5.0
    assert s.take_stale(p.grad) is False and bool((p.grad == 5.0).all())
    q = torch.nn.Parameter(torch.zeros(3))   # fresh without a buffer: the mark is cleared, AccumulateGrad will create .grad
    sq = table_grad.of(q, create=True)
    sq.begin_step()
    sq.returning_through_autograd(q)
    assert sq.fresh is False and q.grad is None


def test_a_tensor_without_a_state_gets_the_inert_one():
    t = torch.zeros(4, requires_grad=True).half()   # (what an fp16-table evaluation passes: a non-leaf copy)
    s = table_grad.of(t)
    assert s is table_grad.of(torch.zeros(1)) and not hasattr(t, "_emer_table") and "_emer_table" not in t.__dict__
    s.count_eval()
    assert s.enter_backward() is False and s.take_stale(torch.ones(2)) is False and s.fresh is False and s.pending_evals == 0
    s.returning_through_autograd(t)
    s.complete(t, True, True)
    for name in TableGrad.__slots__:
        with pytest.raises(AttributeError):
            setattr(s, name, None)
    with pytest.raises(AttributeError):
        s.begin_step()
    with pytest.raises(AttributeError):
        TableGrad().misspelt = 1            # __slots__: a misspelt field is an error, not a silently disabled feature


@pytest.mark.parametrize("F", T.FEATURES)
@pytest.mark.parametrize("n", T.COUNTS)
def test_three_evaluations_of_the_probe_stay_exact(oracle, F, n):
    """tests/test_table_routes_gpu.py expects 2 x and 3 x the oracle's gradient bitwise: 3 abs_sum / g < 2^24 at its shapes"""
    import numpy as np
    meta, _, x, _, dout = T.probe(oracle, F, n)
    ref, abs_sum, _ = oracle.hashgrid_bwd_params_bound(meta, x, dout)
    g = GP.g_params(T.D)
    assert 3.0 * float(abs_sum.max()) / g < 2.0 ** 24
    assert np.array_equal(ref / g, np.round(ref / g))
    GP.exact_f32(3.0 * ref)
    assert T.COUNTS == (65, 257) and all(c in GP.COUNTS and c in GP.HALF_COUNTS for c in T.COUNTS)
