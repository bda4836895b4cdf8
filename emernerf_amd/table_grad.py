"""How a hash table's gradient reaches its buffer: one state object per table parameter (``TableGrad``, under the single attribute
``param._emer_table``) and one decision per backward (``route``).  Host only: nothing here loads the library or computes.

A trainer that owns its gradient buffers (``FlatParams``) does not zero a table's gradient: the owner-computes grid backward
writes every entry exactly once.  Over one step a table's state goes

    begin_step            fresh = True, pending_evals = 0
    every forward         count_eval            (counted only while a hook is set)
    every backward        enter_backward        (the last one of the step fires on_last_backward), then ONE route:
                            direct / direct_split   overwrite .grad, fresh = False
                            add / temp_add          add onto what an earlier backward of the step wrote
                            sliced_autograd / atomic   returning_through_autograd: zero a stale .grad, fresh = False
                          complete              (on_complete, if the step's whole gradient now stands in .grad)
    finish_grads          take_stale            a table that no backward wrote gets its zero gradient; fresh = False

so every table of a group the step trained ends it with fresh False, and every table with pending_evals 0.  A replayed hipGraph
runs none of this: the capturing call leaves that same state behind, and ``take_stale`` is a no-op on the replayed steps."""

ROUTES = ("atomic", "sliced_autograd", "direct", "direct_split", "add", "temp_add")


class TableGrad:
    """fresh: ``.grad`` holds last step's values and the first backward of this step overwrites them.
    pending_evals: counted forward evaluations of this step whose backward has not run yet.
    on_last_backward: f(), the table's last backward of the step starts (everything upstream has its gradient enqueued).
    on_complete: f(param), the step's whole gradient stands in ``.grad``.
    split: (k, f(param, lo, hi)), the last backward runs the levels [k, L), calls f on their range of the table, then [0, k)."""
    __slots__ = ("fresh", "pending_evals", "on_last_backward", "on_complete", "split")

    def __init__(self):
        self.fresh, self.pending_evals = False, 0
        self.on_last_backward = self.on_complete = self.split = None

    def begin_step(self) -> None:
        """The trainer's zero_grad for a table: mark instead of zeroing.  (A forward without a backward -- an eval render between
        steps -- must not shift the count.)"""
        self.fresh, self.pending_evals = True, 0

    def count_eval(self) -> None:
        """An encoder evaluated more than once per step (warped positions, chunked training) runs its LAST backward for its FIRST
        forward: the evaluations are counted so that the hooks fire exactly then."""
        if self.on_last_backward is not None or self.on_complete is not None:
            self.pending_evals += 1

    def enter_backward(self) -> bool:
        """-> True when this is the table's last backward of the step (and a hook asked to know)."""
        if self.on_last_backward is None and self.on_complete is None:
            return False
        self.pending_evals = left = max(self.pending_evals - 1, 0)
        if left == 0 and self.on_last_backward is not None:
            self.on_last_backward()
        return left == 0

    def complete(self, param, last: bool, in_place: bool) -> None:
        """``in_place``: this backward wrote or added the gradient in the trainer's buffer, it did not hand it to AccumulateGrad."""
        if self.on_complete is not None and last and in_place:
            self.on_complete(param)

    def take_stale(self, grad_view) -> bool:
        """No backward wrote the table this step: zero its buffer (if it has one) now, before anything reads it."""
        if not self.fresh:
            return False
        if grad_view is not None:
            grad_view.zero_()
        self.fresh = False
        return True

    def returning_through_autograd(self, param) -> None:
        """The gradient goes BACK to autograd, whose AccumulateGrad adds it onto ``param.grad``: a stale buffer is zeroed first and
        the mark cleared -- otherwise the sum lands on last step's values and ``take_stale`` later zeroes it (the row-major, atomic
        and fp16 fallbacks once trained with a zero gradient that way)."""
        if self.fresh:
            self.take_stale(param.grad)


class _Inert(TableGrad):
    """The state of a parameter that no trainer manages: never fresh, no hooks, nothing counted.  Shared, so it refuses writes."""
    __slots__ = ()
    # Plain class attributes hide the slots of TableGrad, and without an instance __dict__ there is nowhere else to store a value: reading
    # a field gives the constant, assigning one (begin_step included) raises AttributeError.  Built without __init__, which would assign.
    fresh, pending_evals, on_last_backward, on_complete, split = False, 0, None, None, None


_INERT = object.__new__(_Inert)


def of(param, create: bool = False) -> TableGrad:
    """The state of ``param``: its own (``create=True`` gives it one: whoever sets a field or calls ``begin_step`` owns the table's
    gradient buffer), else the shared inert one, on which every method is a no-op.  Nothing is stored on ``param`` without ``create``."""
    state = getattr(param, "_emer_table", None)
    if state is None and create:
        state = param._emer_table = TableGrad()
    return state or _INERT


def route(sliced: bool, sink: bool, has_grad: bool, fresh: bool, contiguous: bool, last_and_split: bool) -> str:
    """Which way a grid backward produces the table gradient.  Decided in the backward (``fresh`` changes between two evaluations
    of one encoder in a step), once, before any launch.

    | sliced (masks emitted) | sink recorded at forward | .grad present at backward | fresh | .grad contiguous | last and valid split (0 < k < L) | route |
    |---|---|---|---|---|---|---|
    | no  | -   | -   | -   | -   | -   | atomic          |
    | yes | no  | -   | -   | -   | -   | sliced_autograd |
    | yes | yes | no  | -   | -   | -   | sliced_autograd |
    | yes | yes | yes | yes | -   | yes | direct_split    |
    | yes | yes | yes | yes | -   | no  | direct          |
    | yes | yes | yes | no  | yes | -   | add             |
    | yes | yes | yes | no  | no  | -   | temp_add        |

    atomic: zeroed temporary, global atomics, back through autograd.  sliced_autograd: owner computes into a temporary, back
    through autograd.  direct: owner computes straight into .grad.  direct_split: the same in two level-range launches with the
    split's hook between them.  add: the accumulating kernel onto .grad.  temp_add: owner computes into a temporary, then
    ``.grad += temporary`` (only when .grad was replaced by a non-contiguous tensor after the forward recorded the sink)."""
    if not sliced:
        return "atomic"
    if not (sink and has_grad):
        return "sliced_autograd"
    if fresh:
        return "direct_split" if last_and_split else "direct"
    return "add" if contiguous else "temp_add"
