"""Per-ray stages of the colour heads as members of ONE launch (``emer_ray_jobs``, csrc/rayinputs.hip).

The per-ray side of the heads -- input rows, the per-ray pre-activations, the sky head, their weight gradients, the embedding
table's gradient -- touches a few thousand rows.  Members of one launch run side by side.  Measured at 8192 rays (DESIGN.md
4.3b): that pays where a member uses few CUs -- the weight gradients (32 chunks per job) and the embedding gradient (one
workgroup per table row) cost 62 us as three launches and 27 us as one; the row-local stages are 256 full workgroups each and
gain little (in two sessions: front 36.7 / 28.9 us against 37.8 / 37.4 us as four launches, launch A 42.0 / 35.2 us against
43.3 / 43.5 us): for them the job launch mostly saves launches.  This module holds

  * ``emer_ray_job`` and its argument structs (read from the header) and builders for the job kinds,
  * the FRONT launch's parking place: results computed ahead of the Functions that own them (``Front``), picked up by
    identity checks only, exactly like ``fused.RgbRider``,
  * the per-step QUEUE of deferred backward jobs: level A (row-local chains, the reduction of the rgb backward's partials)
    and level B (everything that reads level A's outputs: the weight gradients and the embedding gradient).

The queue is ARMED by a trainer only (``armed()``), for one forward+backward (see ``Trainer._forward_backward``), and a head
defers only when its per-ray input is a live output of ``fused._RayInputsFn`` of that forward (``may_defer``): that producer's
backward is the one consumer of the deferred input gradient and flushes the queue before it reads.  Rows that came any other
way (a torch ``cat`` of encoding and embedding, when the batch has no per-ray indices) have torch consumers that would read the
gradient before it is written: everything else launches at once.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib
from ._lib import CONST, STRUCT, _ptr as _p, _stream

# the switch: EMER_RAY_JOBS=0 (or ENABLED = False) gives the separate launches exactly
ENABLED = os.environ.get("EMER_RAY_JOBS", "1") != "0"

MAX_JOBS = CONST["EMER_RAY_JOBS_MAX"]
INPUTS, PRE_FWD, HEAD_FWD, HEAD_BWD, PRE_BWD, WGRAD, EMBED_GRAD, DW_REDUCE, FWD_CHAIN, BWD_CHAIN = (
    CONST["EMER_RAY_JOB_" + k] for k in ("INPUTS", "PRE_FWD", "HEAD_FWD", "HEAD_BWD", "PRE_BWD", "WGRAD", "EMBED_GRAD", "DW_REDUCE",
                                        "FWD_CHAIN", "BWD_CHAIN"))

# emer_ray_job and the argument structs of its kinds (include/emernerf_hip.h)
InputsArgs, PreFwdArgs, PreBwdArgs, HeadFwdArgs, HeadBwdArgs, EmbedGradArgs, WgradJob, WgradArgs, DwReduceJob, DwReduceArgs, RayJob = (
    STRUCT["emer_" + k] for k in ("ray_inputs_args", "ray_pre_fwd_args", "ray_pre_bwd_args", "ray_head_fwd_args", "ray_head_bwd_args",
                                  "embed_grad_args", "ray_wgrad_job", "ray_wgrad_args", "dw_reduce_job", "dw_reduce_args", "ray_job"))


# ------------------------------------------------------------------------------------------------ builders
def inputs_args(dirs: Tensor, idx: Tensor, w: Tensor, max_deg: int, out_rgb: Optional[Tensor], out_sky: Optional[Tensor]) -> InputsArgs:
    ref = out_rgb if out_rgb is not None else out_sky
    return InputsArgs(_p(dirs), dirs.stride(0), _p(idx), idx.stride(0), _p(w), w.shape[0], w.shape[1], max_deg, 0, dirs.shape[0],
                      _p(out_rgb), ref.stride(0), _p(out_sky), ref.stride(0))


def pre_fwd_args(h: Tensor, W0: Tensor, B0: Optional[Tensor], W1: Tensor, B1: Optional[Tensor], rb: Tensor) -> PreFwdArgs:
    """rb = [W0[:, :Kh] h + b0 | W1[:, H:H+Kh] h + b1] (the weight blocks are read in place)."""
    R, Kh = h.shape
    H = W0.shape[0]
    return PreFwdArgs(_p(h), h.stride(0), R, Kh, H, _p(W0), W0.stride(0), _p(B0), _p(W1[:, H:]), W1.stride(0), _p(B1), _p(rb), rb.stride(0))


def pre_bwd_args(s0: Tensor, s1: Tensor, Kh: int, W0: Tensor, W1: Tensor, dh: Tensor) -> PreBwdArgs:
    R, H = s0.shape
    assert s0.stride(0) == s1.stride(0)
    return PreBwdArgs(_p(s0), _p(s1), s0.stride(0), R, Kh, H, _p(W0), W0.stride(0), _p(W1[:, H:]), W1.stride(0), _p(dh), dh.stride(0))


def head_fwd_args(rb: Tensor, W1: Tensor, W2: Tensor, B2: Optional[Tensor], act: int, a1: Tensor, a2: Tensor, out: Tensor) -> HeadFwdArgs:
    return HeadFwdArgs(_p(rb), rb.stride(0), rb.shape[0], _p(W1), W1.stride(0), _p(W2), _p(B2), W2.shape[0], act, _p(a1), _p(a2), _p(out))


def head_bwd_args(dout: Tensor, out: Tensor, a1: Tensor, a2: Tensor, W1: Tensor, W2: Tensor, act: int, dpre2: Tensor, dpre1: Tensor,
                  dpre0: Tensor) -> HeadBwdArgs:
    return HeadBwdArgs(_p(dout), _p(out), _p(a1), _p(a2), out.shape[0], _p(W1), W1.stride(0), _p(W2), W2.shape[0], act, _p(dpre2), _p(dpre1),
                       _p(dpre0))


def embed_grad_args(ga: Optional[Tensor], lda: int, gb: Optional[Tensor], ldb: int, idx: Tensor, n_emb: int, emb_dim: int, dw: Tensor) -> EmbedGradArgs:
    return EmbedGradArgs(_p(ga), lda, _p(gb), ldb, _p(idx), idx.stride(0), idx.shape[0], n_emb, emb_dim, _p(dw))


def fill_wgrad(a: WgradJob, dy: Tensor, blocks, dw: Tensor, db: Optional[Tensor]) -> None:
    """(dy [M, n], [(x [M, >= width], width, dst_col), ...], dw, dbias | None), as fused.ray_wgrad takes them."""
    M = dy.shape[0]
    assert dy.stride(1) == 1 and dw.stride(1) == 1 and 1 <= len(blocks) <= 2
    a.dy, a.ld_dy, a.n, a.n_segs = dy.data_ptr(), dy.stride(0), dy.shape[1], len(blocks)
    a.dw, a.ld_dw, a.dbias = dw.data_ptr(), dw.stride(0), (None if db is None else db.data_ptr())
    for i, (x, width, dst) in enumerate(blocks):
        assert x.shape[0] == M and x.stride(1) == 1
        a.x[i], a.ld_x[i], a.width[i], a.dst_col[i] = x.data_ptr(), x.stride(0), width, dst


def job(kind: int, args=None, n_stages: int = 1) -> RayJob:
    j = RayJob()
    j.kind, j.n_stages = kind, n_stages
    if args is not None:
        name = {INPUTS: "inputs", PRE_FWD: "pre_fwd", HEAD_FWD: "head_fwd", HEAD_BWD: "head_bwd", PRE_BWD: "pre_bwd", WGRAD: "wgrad",
                EMBED_GRAD: "embed_grad", DW_REDUCE: "dw_reduce"}[kind]
        setattr(j.u, name, args)
    return j


def wgrad_job(dy: Tensor, blocks, dw: Tensor, db: Optional[Tensor]) -> RayJob:
    j = job(WGRAD)
    fill_wgrad(j.u.wgrad.job, dy, blocks, dw, db)
    j.u.wgrad.m = dy.shape[0]
    return j


def fwd_chain_job(inp: InputsArgs, pre: PreFwdArgs, head: Optional[HeadFwdArgs] = None) -> RayJob:
    j = job(FWD_CHAIN, n_stages=2 if head is None else 3)
    j.u.fwd_chain.inp, j.u.fwd_chain.pre = inp, pre
    if head is not None:
        j.u.fwd_chain.head = head
    return j


def bwd_chain_job(head: HeadBwdArgs, pre: PreBwdArgs) -> RayJob:
    j = job(BWD_CHAIN)
    j.u.bwd_chain.head, j.u.bwd_chain.pre = head, pre
    return j


def launch(jobs: List[RayJob], ref: Tensor) -> None:
    """The jobs in as few launches as EMER_RAY_JOBS_MAX allows (one, for every list this package builds), on ``ref``'s device and
    torch's current stream."""
    with torch.cuda.device(ref.device):
        stream = _stream(ref)
        for i in range(0, len(jobs), MAX_JOBS):
            part = jobs[i:i + MAX_JOBS]
            arr = (RayJob * len(part))(*part)
            _lib.call("emer_ray_jobs", arr, len(part), stream)


@contextlib.contextmanager
def capture_dw_reduce(cap: DwReduceArgs):
    """The reduction that the entry point called inside this block would launch is described in ``cap`` instead (cap.n_jobs == 0
    afterwards: it launched none)."""
    cap.n_jobs = 0
    _lib.call("emer_dw_reduce_defer", ctypes.byref(cap))
    try:
        yield cap
    finally:
        _lib.call("emer_dw_reduce_defer", None)


# ------------------------------------------------------------------------------------------------ the front launch's results
class Front:
    """What the front launch computed ahead of its owners.  ``rgb``: (hray, (w0, b0, w1, b1), versions, rb) -- the rgb head's per-ray
    pre-activations; ``sky``: (x, (w0 .. b2), versions, final_act, rb, a1, a2, out) -- the whole sky head.  A later caller takes a
    result only if ITS input is the same storage and shape and ITS parameters are the same objects, unchanged since."""

    def __init__(self):
        self.rgb = None
        self.sky = None


_FRONTS: dict = {}   # data_ptr of an input-row tensor -> Front


def clear_fronts() -> None:
    _FRONTS.clear()


def park(out_rgb: Tensor, out_sky: Tensor, front: Front) -> None:
    if front.rgb is not None:
        _FRONTS[out_rgb.data_ptr()] = front
    if front.sky is not None:
        _FRONTS[out_sky.data_ptr()] = front


def _same(x: Tensor, x0: Tensor, params, params0, versions) -> bool:
    return bool(x.data_ptr() == x0.data_ptr() and x.shape == x0.shape and x.stride() == x0.stride() and len(params) == len(params0)
                and all(a is b for a, b in zip(params, params0)) and all(p._version == v for p, v in zip(params0, versions)))


def front_rb(hray: Tensor, params) -> Optional[Tensor]:
    """The parked per-ray pre-activations of the rgb head for exactly this input and these (w0, b0, w1, b1), or None."""
    f = _FRONTS.get(hray.data_ptr())
    if f is None or f.rgb is None:
        return None
    x0, p0, ver, rb = f.rgb
    return rb if _same(hray, x0, tuple(params), p0, ver) else None


def front_sky(x: Tensor, params, final_act: int):
    """The parked (rb, a1, a2, out) of the sky head for exactly this input and these parameters, or None."""
    f = _FRONTS.get(x.data_ptr())
    if f is None or f.sky is None:
        return None
    x0, p0, ver, act, res = f.sky
    return res if (act == final_act and _same(x, x0, tuple(params), p0, ver)) else None


# ------------------------------------------------------------------------------------------------ the deferred tail
class _Queue:
    def __init__(self):
        self.a: List[RayJob] = []      # first level: row-local chains, the reduction of the rgb backward's partials
        self.b: List[RayJob] = []      # second level: reads what the first level writes
        self.keep: list = []           # every tensor a queued job points into
        self.ref: Optional[Tensor] = None
        self.rows: dict = {}           # data_ptr -> tensor: the live outputs of fused._RayInputsFn of this forward (kept alive: no reuse)
        self.deferred: dict = {}       # data_ptr of a head's per-ray INPUT -> its gradient tensor, which the queue has yet to write


_QUEUE: Optional[_Queue] = None


def armed() -> bool:
    return _QUEUE is not None


def register_rows(*rows: Tensor) -> None:
    """fused._RayInputsFn.forward: these tensors are its outputs -- the only per-ray inputs whose gradient may be deferred."""
    q = _QUEUE
    if q is not None:
        for t in rows:
            q.rows[t.data_ptr()] = t


def may_defer(x: Tensor) -> bool:
    """Whether a head whose per-ray input is ``x`` may queue its backward jobs: the queue is armed and ``x`` is, storage, shape
    and strides, a registered output of fused._RayInputsFn of this forward+backward."""
    q = _QUEUE
    if q is None:
        return False
    t = q.rows.get(x.data_ptr())
    return t is not None and t.shape == x.shape and t.stride() == x.stride()


def pending() -> int:
    return 0 if _QUEUE is None else len(_QUEUE.a) + len(_QUEUE.b)


@contextlib.contextmanager
def deferred_tail(enabled: bool = True):
    """Arm the queue for one forward+backward.  The CALLER guarantees that every input gradient a queued job writes goes to one
    consumer that flushes first (fused._RayInputsFn.backward) and that nothing reads a weight gradient before ``flush``."""
    global _QUEUE
    prev = _QUEUE
    _QUEUE = _Queue() if (enabled and ENABLED) else None
    try:
        yield
        flush()
    finally:
        _QUEUE = prev


def enqueue(level_a: List[RayJob], level_b: List[RayJob], keep, ref: Tensor, outputs=()) -> None:
    q = _QUEUE
    assert q is not None
    for _, x in outputs:
        assert may_defer(x), "ray_jobs: a deferred input gradient must belong to an output of fused._RayInputsFn of this forward"
    q.a += level_a
    q.b += level_b
    q.keep.append(keep)
    q.ref = ref
    for grad, x in outputs:   # (the gradient tensor the jobs will write, the input it is the gradient of)
        q.deferred[x.data_ptr()] = grad


def check_single_consumer(input_ptr: int, g: Optional[Tensor]) -> None:
    """Called by the producer of a head's per-ray input with the gradient autograd handed it: if a head deferred the jobs that
    write that input's gradient, ``g`` must BE the tensor those jobs write.  Anything else (a sum autograd formed because the
    input had a second consumer, a copy) was computed from memory that is not written yet."""
    q = _QUEUE
    d = None if q is None else q.deferred.get(input_ptr)
    if d is None:
        return
    if g is None or g.data_ptr() != d.data_ptr() or g.shape != d.shape or g.stride() != d.stride():
        raise RuntimeError("ray_jobs: a deferred per-ray input gradient did not reach its producer as the one gradient of that input "
                           "(the input has more than one consumer): the deferred tail must not be armed for this model")


def flush(extra_b: Optional[List[RayJob]] = None, ref: Optional[Tensor] = None) -> None:
    """Launch A, then launch B (with ``extra_b`` appended): no-op when nothing is queued."""
    q = _QUEUE
    a, b = ([], []) if q is None else (q.a, q.b)
    b = b + (extra_b or [])
    ref = ref if ref is not None else (None if q is None else q.ref)
    if a:
        launch(a, ref)
    if b:
        launch(b, ref)
    if q is not None:
        q.a, q.b, q.keep, q.deferred = [], [], [], {}   # (q.rows stays: a second backward of the same forward)
