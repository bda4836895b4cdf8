"""torch.autograd wrappers over the C-ABI kernels (PyTorch here is plumbing: device memory, streams,
autograd bookkeeping).  Every op launches hand-written HIP through ``_lib.call``; nothing in this
module computes on the CPU or through torch math, so a missing extension fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib, table_grad
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TRUNC_EXP, CONST, F16, F32, GridDesc, STOT_TYPES, STRUCT, _f32c, _ng, _ptr, _stream  # noqa: F401

_ACTS = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "trunc_exp": ACT_TRUNC_EXP}


def _check_cuda(*ts: Tensor):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.EmerError("emernerf_amd ops need GPU (HIP) tensors; there is no CPU fallback")


def _opt(t: Optional[Tensor]) -> Optional[Tensor]:
    """_f32c of an optional tensor (an absent input or gradient stays None: a null pointer for the kernel)."""
    return None if t is None else _f32c(t)


def _empty(ref: Tensor, *shape) -> Tensor:
    """Uninitialised fp32 output on ``ref``'s device."""
    return torch.empty(shape, device=ref.device, dtype=torch.float32)


def _dtype_tag(t: Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise _lib.EmerError(f"unsupported table dtype {t.dtype}")


# ------------------------------------------------------------------------------------ hash grid
MASK_SCRATCH = CONST["EMER_SLICE_MASK_SCRATCH"]  # work cursors (and pacing counters) of the backward behind the bitmaps


def sliced_supported(desc: GridDesc) -> bool:
    """True when the owner-computes LDS backward handles this grid (every level <= 64 LDS slices)."""
    return bool(_lib.load().emer_hashgrid_sliced_supported(ctypes.byref(desc)))


def sliced_split_level(desc) -> int:
    """Level k at which the owner-computes table backward is cut into the launches [k, L) and [0, k) without lengthening it by a
    round of work items (0: do not cut).  See emer_hashgrid_sliced_split_level (csrc/hashgrid.hip)."""
    return int(_lib.load().emer_hashgrid_sliced_split_level(ctypes.byref(desc)))


def mask_words(desc: GridDesc, n: int) -> int:
    """64-bit words of the slice bitmaps for n samples: n_levels x rows x ceil(n / 64) + the backward's work cursors
    (rows = 64, or 256 for tables with more than 64 LDS slices per level: emer_hashgrid_mask_rows)."""
    rows = int(_lib.load().emer_hashgrid_mask_rows(ctypes.byref(desc)))
    if rows <= 0:
        raise _lib.EmerError("slice bitmaps requested for a grid the owner-computes backward does not support")
    return desc.n_levels * rows * ((n + 63) // 64) + MASK_SCRATCH


def hashgrid_fwd_raw(desc: GridDesc, x: Tensor, params: Tensor, level_major: bool = True, want_masks: bool = False, jac_row0=None):
    """Encode; returns [L, N, F] (level_major) or [N, L*F] fp32 (and the int64 slice bitmaps, ``mask_words(desc, N)`` long, if asked).
    ``jac_row0`` (fp32 tables): also returns d out / d x of the rows jac_row0 .. N - 1 as [L, N - jac_row0, F, D] (last element of
    the returned tuple) -- see emer_hashgrid_fwd_jac."""
    _check_cuda(x, params)
    N, L, F = x.shape[0], desc.n_levels, desc.n_features
    assert x.shape[1] == desc.n_dims and params.numel() == desc.n_entries * F
    with torch.cuda.device(x.device):
        if level_major:
            out = torch.empty((L, N, F), device=x.device, dtype=torch.float32)
            sn, sl = F, N * F
        else:
            out = torch.empty((N, L * F), device=x.device, dtype=torch.float32)
            sn, sl = L * F, F
        masks = torch.empty((mask_words(desc, N),), device=x.device, dtype=torch.int64) if want_masks else None
        if jac_row0 is None:
            _lib.call("emer_hashgrid_fwd", ctypes.byref(desc), _ptr(x), _ptr(params), _dtype_tag(params), _ptr(out), sn, sl,
                      _ptr(masks), N, _stream(x))
            return (out, masks) if want_masks else out
        assert params.dtype == torch.float32 and 0 <= jac_row0 <= N
        jac = torch.empty((L, N - jac_row0, F, desc.n_dims), device=x.device, dtype=torch.float32)
        _lib.call("emer_hashgrid_fwd_jac", ctypes.byref(desc), _ptr(x), _ptr(params), _ptr(out), sn, sl, _ptr(masks), _ptr(jac),
                  int(jac_row0), N, _stream(x))
    return (out, masks, jac) if want_masks else (out, jac)


# [r4] input gradient of a grid encoding (the flow configs: warped positions) from the Jacobians the forward stores instead of a second
# gather pass over the table (emer_hashgrid_bwd_input): -0.4 ms per flow step at 2048 rays.  EMER_GRID_JAC=0: the gather pass.
GRID_JAC = os.environ.get("EMER_GRID_JAC", "1") != "0"
# The Jacobian is L * F * D * 4 bytes per row that needs dx (640 B for the D4/L10/F4 xyzt tables), held from the forward to the backward
# (under capture: in the graph's pool).  Evaluations whose Jacobian would exceed this budget take the gather pass instead, so a ray batch
# that fitted before the Jacobian path existed still fits.  EMER_GRID_JAC_MAX_MB=0: no limit.
GRID_JAC_MAX_BYTES = int(float(os.environ.get("EMER_GRID_JAC_MAX_MB", "4096")) * (1 << 20))


def _jac_fits(desc, rows: int) -> bool:
    return GRID_JAC_MAX_BYTES <= 0 or rows * desc.n_levels * desc.n_features * desc.n_dims * 4 <= GRID_JAC_MAX_BYTES


def slice_masks(desc: GridDesc, x: Tensor) -> Tensor:
    _check_cuda(x)
    with torch.cuda.device(x.device):
        masks = torch.empty((mask_words(desc, x.shape[0]),), device=x.device, dtype=torch.int64)
        _lib.call("emer_hashgrid_slice_masks", ctypes.byref(desc), _ptr(x), _ptr(masks), x.shape[0], _stream(x))
    return masks


def layout_transpose(src: Tensor, L: int, N: int, F: int, to_row_major: bool) -> Tensor:
    _check_cuda(src)
    with torch.cuda.device(src.device):
        dst = torch.empty((N, L * F) if to_row_major else (L, N, F), device=src.device, dtype=torch.float32)
        _lib.call("emer_layout_transpose", _ptr(src), _ptr(dst), L, N, F, int(to_row_major), _stream(src))
    return dst


class _LmToRmFn(torch.autograd.Function):
    """Level-major grid encoding [L, N, F] -> the reference's row-major [N, L*F] (differentiable; one transpose kernel)."""

    @staticmethod
    def forward(ctx, enc_lm: Tensor):
        L, N, F = enc_lm.shape
        ctx.shape = (L, N, F)
        return layout_transpose(_f32c(enc_lm), L, N, F, to_row_major=True)

    @staticmethod
    def backward(ctx, dout: Tensor):
        L, N, F = ctx.shape
        return layout_transpose(_f32c(dout), L, N, F, to_row_major=False)


def lm_to_rm(enc_lm: Tensor) -> Tensor:
    return _LmToRmFn.apply(enc_lm)


CHECK_FINITE = os.environ.get("EMER_CHECK_FINITE") == "1"


DEFERRED_FINITE: list = []   # (grid name, N, any-bad flag, flat index of the first bad (level, sample)) recorded during a graph capture


def check_deferred_finite(entries) -> None:
    """Raise FloatingPointError if a replayed graph's recorded checks (see _check_finite_grid_grad) saw a non-finite gradient."""
    for name, n, flag, first in entries:
        if bool(flag):
            i = int(first)
            raise FloatingPointError(f"non-finite gradient entering the {name} hash-grid backward at (level, sample) [{i // n}, {i % n}] "
                                     "(first offender; hipGraph replay)")


def _check_finite_grid_grad(dlm: Tensor, desc: GridDesc) -> None:
    """Debug aid (EMER_CHECK_FINITE=1, the analogue of the reference's optim.check_nan, loss/base.py:77-79).  The owner-computes
    backward reduces runs of equal cells with 0/1-masked multiply-adds, so ONE non-finite entry of the incoming gradient
    contaminates other table entries of its wave (0 x inf = NaN; upstream's atomics keep it in the sample's own cells): looking
    at the table gradient afterwards points at the wrong entries.  This check names the offending (level, sample) pairs BEFORE
    the scatter; it costs one reduction over the gradient and a host read, so it is off by default.  While a hipGraph is being
    captured the verdict is left on the device and read after each replay (``check_deferred_finite``)."""
    if torch.cuda.is_current_stream_capturing():
        # a host read cannot be captured: the verdict stays on the device (tensors of the graph's pool, rewritten by every replay)
        # and the owner of the graph reads it after g.replay() (check_deferred_finite; Trainer does when CHECK_FINITE is on)
        per = (~torch.isfinite(dlm)).any(dim=-1).view(-1)                      # [L * N]
        DEFERRED_FINITE.append((f"D{desc.n_dims}/L{desc.n_levels}/F{desc.n_features}", dlm.shape[1], per.any(), per.to(torch.uint8).argmax()))
        return
    bad = ~torch.isfinite(dlm)
    if bool(bad.any()):
        idx = torch.nonzero(bad.any(dim=-1))[:8].tolist()
        raise FloatingPointError(f"non-finite gradient entering the D{desc.n_dims}/L{desc.n_levels}/F{desc.n_features} hash-grid backward at "
                                 f"(level, sample) {idx}{' ...' if int(bad.any(dim=-1).sum()) > 8 else ''}")


def _fp32_accumulation(gdt, desc: GridDesc) -> bool:
    """The table gradient is summed in fp32: asked for, or half gradients of an ODD feature count (every proposal network has one
    feature per level) -- the packed half2 atomics of emer_hashgrid_bwd_params need an even one, so such a gradient takes the fp32
    routes (owner computes where the grid allows, else fp32 atomics) and is rounded to half once."""
    return gdt == torch.float32 or bool(desc.n_features & 1)


def _grid_forward(ctx, xc: Tensor, pc: Tensor, params: Tensor, desc: GridDesc, grad_dtype, jac_row0=None, sink_of=None):
    """What the forwards of both grid Functions share -> (level-major encoding [L, N, F], Jacobian or None).  ``pc``: the table the
    kernels read, ``params``: the parameter its gradient belongs to.  ``sink_of``: ``fused._sink`` if the table gradient may be written
    straight into ``params.grad`` (asked, and recorded as ``ctx.param``, where the owner-computes backward will run in fp32)."""
    gdt = grad_dtype or torch.float32
    # the forward emits the slice masks of the owner-computes backward when it will be used
    ctx.sliced = bool(ctx.needs_input_grad[1] and _fp32_accumulation(gdt, desc) and sliced_supported(desc))
    res = hashgrid_fwd_raw(desc, xc, pc, level_major=True, want_masks=ctx.sliced, jac_row0=jac_row0)
    res = res if isinstance(res, tuple) else (res,)
    masks = res[1] if ctx.sliced else None
    ctx.desc, ctx.grad_dtype, ctx.master_dtype = desc, grad_dtype, params.dtype
    sink = sink_of(params) if (sink_of is not None and ctx.sliced and gdt == torch.float32) else None
    ctx.param = params if (sink is not None and sink.is_contiguous() and sink.numel() == pc.numel()) else None
    ctx.param_obj, ctx.table_route = params, None
    table_grad.of(params).count_eval()
    ctx.save_for_backward(xc, pc, masks)
    return res[0], (res[-1] if jac_row0 is not None else None)


def _enter_grid_backward(ctx, masks) -> None:
    """First thing in both backwards, before any launch: the table's evaluation count (a data-parallel trainer's early bucket
    fires on the table's last backward of the step) and the route of the table gradient (table_grad.route), once."""
    state = table_grad.of(ctx.param_obj)
    ctx.last = state.enter_backward()
    if ctx.needs_input_grad[1]:
        g = None if ctx.param is None else ctx.param.grad
        # (the cut is taken only by the table's LAST backward of the step: an earlier one would start the collective of a range
        # that a later backward of the same table still adds to)
        k = state.split[0] if (ctx.last and state.split is not None) else 0
        ctx.table_route = table_grad.route(sliced=masks is not None, sink=ctx.param is not None, has_grad=g is not None, fresh=state.fresh,
                                           contiguous=g is not None and g.is_contiguous(), last_and_split=0 < k < ctx.desc.n_levels)


def _table_gradient(ctx, desc: GridDesc, xc: Tensor, dlm: Tensor, masks, pc: Tensor, st):
    """Run ``ctx.table_route`` (level-major ``dlm``) -> the gradient to hand back to autograd, None where it went into ``.grad``."""
    N, L, F = xc.shape[0], desc.n_levels, desc.n_features
    route, param, state = ctx.table_route, ctx.param, table_grad.of(ctx.param_obj)
    gdt = ctx.grad_dtype or torch.float32
    grad = None
    if route == "atomic":  # tcnn-style global atomics: fp16-gradient mode, or tables too large for the LDS slices
        grad = torch.zeros(pc.numel(), device=xc.device, dtype=torch.float32 if _fp32_accumulation(gdt, desc) else gdt)
        _lib.call("emer_hashgrid_bwd_params", ctypes.byref(desc), _ptr(xc), _ptr(dlm), F, N * F, _ptr(grad), _dtype_tag(grad), N, st)
    elif route == "direct_split":
        # data-parallel trainer: the levels [k, L) first, then ITS hook (the collective of that contiguous range of the table starts
        # on the communication stream), then the levels [0, k) while it runs
        (k, hook), buf = state.split, param.grad.view(-1)
        _lib.call("emer_hashgrid_bwd_params_sliced_levels", ctypes.byref(desc), _ptr(xc), _ptr(dlm), F, N * F, _ptr(masks), _ptr(buf), N, k, L, st)
        hook(param, int(desc.offset[k]) * F, pc.numel())
        _lib.call("emer_hashgrid_bwd_params_sliced_levels", ctypes.byref(desc), _ptr(xc), _ptr(dlm), F, N * F, _ptr(masks), _ptr(buf), N, 0, k, st)
    else:
        # owner-computes LDS scatter: writes every entry once (no memset, no global atomics) -- straight into .grad ("direct"), [r5]
        # added onto it in the write-out by a further evaluation of the same encoder in this step ("add"), or into a temporary
        buf = param.grad.view(-1) if route in ("direct", "add") else torch.empty(pc.numel(), device=xc.device, dtype=torch.float32)
        _lib.call("emer_hashgrid_bwd_params_sliced_add" if route == "add" else "emer_hashgrid_bwd_params_sliced", ctypes.byref(desc), _ptr(xc),
                  _ptr(dlm), F, N * F, _ptr(masks), _ptr(buf), N, st)
        if route == "temp_add":
            param.grad.view(-1).add_(buf)
        elif route == "sliced_autograd":
            grad = buf
    if route in ("direct", "direct_split"):
        state.fresh = False
    if grad is not None:
        grad = grad.to(gdt).to(ctx.master_dtype)  # (half gradients of an odd feature count: summed in fp32, rounded once)
        state.returning_through_autograd(ctx.param_obj)
    state.complete(ctx.param_obj, ctx.last, grad is None)
    return grad


class _HashGridFn(torch.autograd.Function):
    """tcnn ``_module_function`` (third_party/tcnn_modules.py:115-174) on HIP.

    The grid kernels run level-major (coalesced); the row-major [N, L*F] tensor the reference API
    returns is produced / consumed through the LDS transpose kernel.
    """

    @staticmethod
    def forward(ctx, x: Tensor, params: Tensor, desc: GridDesc, grad_dtype):
        xc, pc = _f32c(x), params.detach().contiguous()
        lm, _ = _grid_forward(ctx, xc, pc, params, desc, grad_dtype)   # (no sink: its table gradient always returns through autograd)
        return layout_transpose(lm, desc.n_levels, xc.shape[0], desc.n_features, to_row_major=True)

    @staticmethod
    def backward(ctx, dout: Tensor):
        xc, pc, masks = ctx.saved_tensors
        desc = ctx.desc
        N, L, F = xc.shape[0], desc.n_levels, desc.n_features
        dx = dp = None
        _enter_grid_backward(ctx, masks)
        with torch.cuda.device(xc.device):
            dlm = layout_transpose(_f32c(dout), L, N, F, to_row_major=False)
            st = _stream(xc)
            if ctx.needs_input_grad[1]:
                dp = _table_gradient(ctx, desc, xc, dlm, masks, pc, st)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(xc)
                _lib.call("emer_hashgrid_bwd_input", ctypes.byref(desc), _ptr(xc), _ptr(pc), _dtype_tag(pc), _ptr(dlm), F,
                          N * F, _ptr(dx), N, st)
        return dx, dp, None, None


class _HashGridLMFn(torch.autograd.Function):
    """Same as _HashGridFn but exchanges the LEVEL-MAJOR [L, N, F] tensors the grid kernels use natively
    (no transpose kernels): what the fused MLP chains read and write.

    Gradient sink (``fused.grad_sinks()``, a trainer that owns its gradient buffers): the owner-computes backward writes
    every table entry exactly once, so it can write STRAIGHT into the parameter's ``.grad`` -- no 49 MB temporary, no
    AccumulateGrad add, and the trainer does not zero the table's gradient beforehand (its zero_grad marks the table's state
    ``fresh``, table_grad.py: the first backward of a step overwrites, later ones of the same step -- the flow configs evaluate
    an encoder three times -- add).  Which of the six routes a backward took: ``out.grad_fn.table_route``.

    ``table_dtype=torch.float16`` with an fp32 ``params``: half-precision tables the way BASELINE.md 2.2 / tcnn run them --
    the fp32 MASTER is cast to fp16 for this call (emer_cast_f32_f16), the encode and the input gradient read the fp16 copy
    (half the gather bytes), and the gradient is accumulated in fp32 by the owner-computes backward (which never reads the
    table) straight into the master's ``.grad``.  ``skip_dx_rows``: leading rows of ``x`` that carry no gradient (the current
    positions in a batched [current | warped | warped] evaluation): the input-gradient kernel skips them."""

    @staticmethod
    def forward(ctx, x: Tensor, params: Tensor, desc: GridDesc, grad_dtype, table_dtype=None, skip_dx_rows: int = 0):
        xc, pc = _f32c(x), params.detach().contiguous()
        if table_dtype == torch.float16 and pc.dtype == torch.float32:
            ph = torch.empty(pc.shape, device=pc.device, dtype=torch.float16)
            with torch.cuda.device(pc.device):
                _lib.call("emer_cast_f32_f16", _ptr(pc), _ptr(ph), pc.numel(), _stream(pc))
            pc = ph  # what the kernels read; `params` stays the fp32 master (gradient sink)
        k = min(int(skip_dx_rows), xc.shape[0])
        want_jac = GRID_JAC and ctx.needs_input_grad[0] and pc.dtype == torch.float32 and k < xc.shape[0] and _jac_fits(desc, xc.shape[0] - k)
        # (the Jacobian not through save_for_backward: never an input or output of the function, freed with the node)
        from . import fused
        lm, ctx.jac = _grid_forward(ctx, xc, pc, params, desc, grad_dtype, jac_row0=k if want_jac else None, sink_of=fused._sink)
        ctx.skip_dx_rows = int(skip_dx_rows)
        return lm

    @staticmethod
    def backward(ctx, dlm: Tensor):
        xc, pc, masks = ctx.saved_tensors
        desc = ctx.desc
        N, L, F = xc.shape[0], desc.n_levels, desc.n_features
        dx = dp = None
        _enter_grid_backward(ctx, masks)
        with torch.cuda.device(xc.device):
            dlm = _f32c(dlm)
            if CHECK_FINITE:
                _check_finite_grid_grad(dlm, desc)
            st = _stream(xc)
            if ctx.needs_input_grad[1]:
                dp = _table_gradient(ctx, desc, xc, dlm, masks, pc, st)
            if ctx.needs_input_grad[0]:
                k, D = min(ctx.skip_dx_rows, N), desc.n_dims
                dx = torch.empty_like(xc)
                if k > 0:
                    dx[:k].zero_()  # rows without a consumer (torch.cat's backward slices them away)
                if N > k and ctx.jac is not None:
                    _lib.call("emer_hashgrid_bwd_input_jac", ctypes.byref(desc), _ptr(ctx.jac), dlm.data_ptr() + 4 * k * F, F, N * F,
                              dx.data_ptr() + 4 * k * D, N - k, st)
                    ctx.jac = None
                elif N > k:  # level-major dlm [L][N][F]: row k of every level is k*F floats in, the level stride stays N*F
                    _lib.call("emer_hashgrid_bwd_input", ctypes.byref(desc), xc.data_ptr() + 4 * k * D, _ptr(pc), _dtype_tag(pc),
                              dlm.data_ptr() + 4 * k * F, F, N * F, dx.data_ptr() + 4 * k * D, N - k, st)
        return dx, dp, None, None, None, None


def hashgrid_encode_lm(x: Tensor, params: Tensor, desc: GridDesc, grad_dtype=None, table_dtype=None, skip_dx_rows: int = 0) -> Tensor:
    """x [N,D] in [0,1] -> level-major [L, N, F] fp32, differentiable w.r.t. params and x (see _HashGridLMFn for
    ``table_dtype`` / ``skip_dx_rows``)."""
    return _HashGridLMFn.apply(*_ng(x, params, desc, grad_dtype, table_dtype, skip_dx_rows))


def hashgrid_encode(x: Tensor, params: Tensor, desc: GridDesc, grad_dtype=None) -> Tensor:
    """x [N,D] in [0,1] -> [N, L*F] fp32, differentiable w.r.t. params and x."""
    return _HashGridFn.apply(*_ng(x, params, desc, grad_dtype))


# ------------------------------------------------------------------------------ contraction
class _ContractFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos: Tensor, aabb: Tensor, unbounded: bool):
        pc = _f32c(pos).view(-1, 3)
        ab = _f32c(aabb).view(-1)
        with torch.cuda.device(pc.device):
            out = torch.empty_like(pc)
            _lib.call("emer_contract_fwd", _ptr(pc), _ptr(ab), int(unbounded), _ptr(out), pc.shape[0], _stream(pc))
        ctx.save_for_backward(pc, ab)
        ctx.unbounded, ctx.shape = unbounded, pos.shape
        return out.view(pos.shape)

    @staticmethod
    def backward(ctx, dout: Tensor):
        pc, ab = ctx.saved_tensors
        dc = _f32c(dout).view(-1, 3)
        with torch.cuda.device(pc.device):
            dpos = torch.empty_like(pc)
            _lib.call("emer_contract_bwd", _ptr(pc), _ptr(ab), int(ctx.unbounded), _ptr(dc), _ptr(dpos), pc.shape[0],
                      _stream(pc))
        return dpos.view(ctx.shape), None, None


def contract_points(pos: Tensor, aabb: Tensor, unbounded: bool) -> Tensor:
    """contract() + selector zeroing (nerf_utils.py:13-28, radiance_field.py:278-300)."""
    _check_cuda(pos, aabb)
    return _ContractFn.apply(pos, aabb, unbounded)


class _FlowWarpFn(torch.autograd.Function):
    """(x3 [3N, 4], x2 [2N, 4]) = xyzt query points of the batched flow branch (radiance_field.py:567-580), see emer_flow_warp_fwd;
    gradient only w.r.t. ``flow`` [N, 6] (positions, timestamps and noise are inputs of the step)."""

    @staticmethod
    def forward(ctx, positions: Tensor, normed: Tensor, ts: Tensor, flow: Tensor, noise: Tensor, time_diff: float, aabb: Tensor, unbounded: bool):
        pos, nrm, t, fl, nz, ab = _f32c(positions).view(-1, 3), _f32c(normed).view(-1, 3), _f32c(ts).view(-1), _f32c(flow).view(-1, 6), \
            _f32c(noise).view(-1), _f32c(aabb).view(-1)
        N = pos.shape[0]
        assert nrm.shape[0] == N and t.numel() == N and fl.shape[0] == N and nz.numel() == N
        with torch.cuda.device(pos.device):
            x3 = torch.empty((3 * N, 4), device=pos.device, dtype=torch.float32)
            x2 = torch.empty((2 * N, 4), device=pos.device, dtype=torch.float32)
            _lib.call("emer_flow_warp_fwd", _ptr(pos), _ptr(nrm), _ptr(t), _ptr(fl), _ptr(nz), float(time_diff), _ptr(ab), int(unbounded), _ptr(x3),
                      _ptr(x2), N, _stream(pos))
        ctx.save_for_backward(pos, fl, nz, ab)
        ctx.unbounded, ctx.flow_shape = bool(unbounded), flow.shape
        return x3, x2

    @staticmethod
    def backward(ctx, dx3: Optional[Tensor], dx2: Optional[Tensor]):
        pos, fl, nz, ab = ctx.saved_tensors
        if not ctx.needs_input_grad[3] or (dx3 is None and dx2 is None):
            return (None,) * 8
        N = pos.shape[0]
        d3 = None if dx3 is None else _f32c(dx3)
        d2 = None if dx2 is None else _f32c(dx2)
        with torch.cuda.device(pos.device):
            dflow = torch.empty((N, 6), device=pos.device, dtype=torch.float32)
            _lib.call("emer_flow_warp_bwd", _ptr(pos), _ptr(fl), _ptr(nz), _ptr(ab), int(ctx.unbounded), _ptr(d3), _ptr(d2), _ptr(dflow), N, _stream(pos))
        return None, None, None, dflow.view(ctx.flow_shape), None, None, None, None


def flow_warp(positions: Tensor, normed: Tensor, timestamps: Tensor, flow: Tensor, noise: Tensor, time_diff: float, aabb: Tensor,
              unbounded: bool) -> Tuple[Tensor, Tensor]:
    """Query points of the flow branch's three xyzt evaluations in one launch: x3 = [current | forward-warped | backward-warped] (the
    dynamic table's batch) and x2 = its last two thirds (the flow table's batch)."""
    _check_cuda(positions, normed, timestamps, flow, noise, aabb)
    return _FlowWarpFn.apply(positions, normed, timestamps, flow, noise, time_diff, aabb, unbounded)


def ray_points(origins: Tensor, dirs: Tensor, t_starts: Tensor, t_ends: Tensor, aabb: Tensor, unbounded: bool,
               times: Optional[Tensor] = None, want_positions: bool = False) -> Tuple[Tensor, Optional[Tensor]]:
    """Sample positions along rays, contracted (no grad: sample positions never carry grad,
    nerfacc_prop_net.py:89).  Returns (normed [R,S,3|4], positions [R,S,3] | None)."""
    _check_cuda(origins, dirs, t_starts, t_ends, aabb)
    R, S = t_starts.shape
    o, d, ts, te, ab = _f32c(origins), _f32c(dirs), _f32c(t_starts), _f32c(t_ends), _f32c(aabb).view(-1)
    tm = None if times is None else _f32c(times).view(-1)
    od = 3 if tm is None else 4
    with torch.cuda.device(o.device):
        normed = torch.empty((R, S, od), device=o.device, dtype=torch.float32)
        pos = torch.empty((R, S, 3), device=o.device, dtype=torch.float32) if want_positions else None
        _lib.call("emer_ray_points", _ptr(o), _ptr(d), _ptr(ts), _ptr(te), _ptr(tm), _ptr(ab), int(unbounded), _ptr(normed),
                  od, _ptr(pos), R, S, _stream(o))
    return normed, pos


# ---------------------------------------------------------------------------------- sampler
SAMPLE_POINTS = os.environ.get("EMER_FUSE_SAMPLE_POINTS", "1") != "0"   # [r5] sampler + sample points in one launch (importance_sample(points=...))
_SAMPLE_POINTS_CAP = None


def sample_points_capacity() -> int:
    """Floats of LDS per ray the fused sampler + points launch may use (2 m + n + 1 must fit): asked from the device once
    (emer_importance_sample_points_capacity; 10240 on gfx950)."""
    global _SAMPLE_POINTS_CAP
    if _SAMPLE_POINTS_CAP is None:
        _SAMPLE_POINTS_CAP = int(_lib.load().emer_importance_sample_points_capacity())
    return _SAMPLE_POINTS_CAP


def importance_sample(vals: Tensor, cdfs: Tensor, n_intervals: int, jitter: Optional[Tensor] = None,
                      stot: Optional[Tuple[float, float, str]] = None, intervals: bool = False, points=None):
    """nerfacc.pdf.importance_sampling (batched).  Returns (s_edges [R,n+1], t_edges | None), or with
    ``intervals=True`` (s_edges, t_starts [R,n], t_ends [R,n]) written directly by the kernel (no slicing copies).
    ``points=(origins, dirs, aabb, unbounded, want_positions)`` with ``intervals=True``: the launch also computes the new intervals' sample
    points (what ``ray_points`` would from its result, bitwise) and returns (s_edges, t_starts, t_ends, normed [R,n,3], positions | None)."""
    _check_cuda(vals, cdfs)
    v, c = _f32c(vals), _f32c(cdfs)
    R, m = v.shape
    j = None if jitter is None else _f32c(jitter).view(-1)
    if j is not None:
        assert j.numel() == R
    assert not intervals or stot is not None
    if points is not None:
        assert intervals, "points are computed for the interval form"
        origins, dirs, aabb, unbounded, want_pos = points
        o, d, ab = _f32c(origins), _f32c(dirs), _f32c(aabb).view(-1)
        assert o.shape == (R, 3) and d.shape == (R, 3)
        with torch.cuda.device(v.device):
            s_out = torch.empty((R, n_intervals + 1), device=v.device, dtype=torch.float32)
            t_out = torch.empty((R, n_intervals), device=v.device, dtype=torch.float32)
            t_end = torch.empty_like(t_out)
            normed = torch.empty((R, n_intervals, 3), device=v.device, dtype=torch.float32)
            pos = torch.empty((R, n_intervals, 3), device=v.device, dtype=torch.float32) if want_pos else None
            t_min, t_max, typ = stot
            _lib.call("emer_importance_sample_points", _ptr(v), _ptr(c), R, m, n_intervals, _ptr(j), _ptr(s_out), _ptr(t_out), _ptr(t_end),
                      float(t_min), float(t_max), STOT_TYPES[typ], _ptr(o), _ptr(d), _ptr(ab), int(unbounded), _ptr(normed), _ptr(pos), _stream(v))
        return s_out, t_out, t_end, normed, pos
    with torch.cuda.device(v.device):
        s_out = torch.empty((R, n_intervals + 1), device=v.device, dtype=torch.float32)
        if intervals:
            t_out = torch.empty((R, n_intervals), device=v.device, dtype=torch.float32)
            t_end = torch.empty_like(t_out)
        else:
            t_out, t_end = (torch.empty_like(s_out) if stot is not None else None), None
        t_min, t_max, typ = stot if stot is not None else (0.0, 1.0, "uniform")
        _lib.call("emer_importance_sample", _ptr(v), _ptr(c), R, m, n_intervals, _ptr(j), _ptr(s_out), _ptr(t_out), _ptr(t_end),
                  float(t_min), float(t_max), STOT_TYPES[typ], _stream(v))
    return (s_out, t_out, t_end) if intervals else (s_out, t_out)


def stot(s: Tensor, t_min: float, t_max: float, transform_type: str) -> Tensor:
    _check_cuda(s)
    sc = _f32c(s)
    with torch.cuda.device(sc.device):
        t = torch.empty_like(sc)
        _lib.call("emer_stot", _ptr(sc), sc.numel(), float(t_min), float(t_max), STOT_TYPES[transform_type], _ptr(t),
                  _stream(sc))
    return t


# ------------------------------------------------------------------------- proposal supervision
class _PropLevelLossFn(torch.autograd.Function):
    """One proposal level of PropNetEstimator.compute_loss (nerfacc_prop_net.py:181-238): scalar loss (already
    multiplied by ``scale``) with its gradient w.r.t. the level's cdf computed in the same launch."""

    @staticmethod
    def forward(ctx, s_final: Tensor, trans: Tensor, s_prop: Tensor, cdf_prop: Tensor, pulse: float, anti_aliased: bool,
                scale: float):
        sf, tr, sp, cp = _f32c(s_final), _f32c(trans), _f32c(s_prop), _f32c(cdf_prop)
        R, n = tr.shape
        m = cp.shape[1] - 1
        assert sf.shape == (R, n + 1) and sp.shape == (R, m + 1)
        want_grad = ctx.needs_input_grad[3]
        with torch.cuda.device(tr.device):
            rays = torch.empty((R,), device=tr.device, dtype=torch.float32)
            loss = torch.empty((), device=tr.device, dtype=torch.float32)
            dcp = torch.empty_like(cp) if want_grad else None
            _lib.call("emer_prop_loss", _ptr(sf), _ptr(tr), n, _ptr(sp), _ptr(cp), m, float(pulse), int(anti_aliased), R, float(scale),
                      _ptr(rays), _ptr(loss), 0, _ptr(dcp), _stream(tr))
        ctx.save_for_backward(dcp)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        (dcp,) = ctx.saved_tensors
        if dcp is None:
            return (None,) * 7
        gc = _f32c(g).reshape(1)
        with torch.cuda.device(dcp.device):
            out = torch.empty_like(dcp)
            _lib.call("emer_scale", _ptr(dcp), _ptr(gc), 1.0, _ptr(out), dcp.numel(), _stream(dcp))
        return None, None, None, out, None, None, None


def prop_level_loss(s_final: Tensor, trans: Tensor, s_prop: Tensor, cdf_prop: Tensor, pulse: float, anti_aliased: bool,
                    scale: float) -> Tensor:
    """scale * sum over rays and intervals of the interlevel loss of one proposal level (0-dim tensor)."""
    _check_cuda(s_final, trans, s_prop, cdf_prop)
    return _PropLevelLossFn.apply(s_final, trans, s_prop, cdf_prop, pulse, anti_aliased, scale)


# ------------------------------------------------------------------------------- compositing
class _RenderWeightsFn(torch.autograd.Function):
    """(weights, trans, alphas, cdfs, ray_stats[, t_mid, t_dist]) from density; grads flow to sigma only (from every
    differentiable output)."""

    @staticmethod
    def forward(ctx, t_starts: Tensor, t_ends: Tensor, sigma: Tensor, want_t: bool):
        ctx.set_materialize_grads(False)
        ts, te, sg = _f32c(t_starts), _f32c(t_ends), _f32c(sigma)
        R, S = sg.shape
        with torch.cuda.device(sg.device):
            w, T, a = (torch.empty_like(sg) for _ in range(3))
            cdfs, stats = _empty(sg, R, S + 1), _empty(sg, R, 4)
            tm, td = (torch.empty_like(sg), torch.empty_like(sg)) if want_t else (None, None)
            _lib.call("emer_render_weights_fwd", _ptr(ts), _ptr(te), _ptr(sg), R, S, _ptr(w), _ptr(T), _ptr(a), _ptr(cdfs),
                      _ptr(stats), _ptr(tm), _ptr(td), _stream(sg))
        ctx.save_for_backward(ts, te, sg)
        if want_t:
            ctx.mark_non_differentiable(tm, td)
            return w, T, a, cdfs, stats, tm, td
        return w, T, a, cdfs, stats

    @staticmethod
    def backward(ctx, dw, dT, da, dcdfs, dstats, *_unused):
        ts, te, sg = ctx.saved_tensors
        R, S = sg.shape
        gw, gT, ga, gs = _opt(dw), _opt(dT), _opt(da), _opt(dstats)  # gs [R,4]: the kernel reads columns 0, 1
        if dcdfs is not None:  # cdfs = 1 - [T, 0]
            g = -_f32c(dcdfs)[:, :S]
            gT = g.contiguous() if gT is None else gT + g
        if gw is None and gT is None and gs is None and ga is None:
            return None, None, None, None
        with torch.cuda.device(sg.device):
            dsig = torch.empty_like(sg)
            _lib.call("emer_render_weights_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(gw), _ptr(gT), _ptr(ga), _ptr(gs), R, S, _ptr(dsig),
                      _stream(sg))
        return None, None, dsig, None


def render_weights(t_starts: Tensor, t_ends: Tensor, sigma: Tensor, want_t: bool = False):
    """Returns (weights, trans, alphas, cdfs [R,S+1], ray_stats [R,4] = (sum w, sum w*mid, median_depth, 0)) and, with
    ``want_t``, also (t_mid, t_dist) = ((t_starts + t_ends) / 2, t_ends - t_starts) from the same launch."""
    _check_cuda(t_starts, t_ends, sigma)
    return _RenderWeightsFn.apply(t_starts, t_ends, sigma, want_t)


class _CompositeRgbFn(torch.autograd.Function):
    """[r4] ``rendering`` of a model with one density and one colour per sample (render_utils.py:73-122,158-159,217-220) as one launch
    each way: (weights, trans, t_vals, t_dist, opacity [R,1], depth [R,1], median_depth [R,1], rgb [R,3] | None).  Same values as
    render_weights -> accumulate_along_rays -> ray_epilogue (bitwise: tests/test_kernels_gpu.py); ``rgb`` None: geometry only."""

    @staticmethod
    def forward(ctx, t_starts: Tensor, t_ends: Tensor, sigma: Tensor, rgb: Optional[Tensor], rgb_sky: Optional[Tensor]):
        ctx.set_materialize_grads(False)
        ts, te, sg = _f32c(t_starts), _f32c(t_ends), _f32c(sigma)
        R, S = sg.shape
        c = None if rgb is None else _f32c(rgb).reshape(R, S, 3)
        sk = None if (rgb_sky is None or rgb is None) else _f32c(rgb_sky).reshape(R, 3)
        with torch.cuda.device(sg.device):
            w, T, tm, td = (torch.empty_like(sg) for _ in range(4))
            stats = _empty(sg, R, 4)
            opa, dep, med = (_empty(sg, R, 1) for _ in range(3))
            out = _empty(sg, R, 3) if c is not None else None
            _lib.call("emer_composite_rgb_fwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(c), _ptr(sk), R, S, _ptr(w), _ptr(T), _ptr(tm), _ptr(td),
                      _ptr(stats), _ptr(opa), _ptr(dep), _ptr(med), _ptr(out), _stream(sg))
        ctx.save_for_backward(ts, te, sg, c, sk, w, stats)
        ctx.mark_non_differentiable(tm, td, med)
        return w, T, tm, td, opa, dep, med, out

    @staticmethod
    def backward(ctx, dw, dT, _dtm, _dtd, dopa, ddep, _dmed, dout):
        ts, te, sg, c, sk, w, stats = ctx.saved_tensors
        R, S = sg.shape
        if all(g is None for g in (dw, dT, dopa, ddep, dout)):
            return None, None, None, None, None
        gw, gT, go, gd, gr = _opt(dw), _opt(dT), _opt(dopa), _opt(ddep), _opt(dout)
        need_rgb = c is not None and ctx.needs_input_grad[3] and gr is not None
        need_sky = sk is not None and ctx.needs_input_grad[4] and gr is not None
        with torch.cuda.device(sg.device):
            dsig = torch.empty_like(sg)
            drgb = torch.empty_like(c) if need_rgb else None
            dsky = torch.empty_like(sk) if need_sky else None
            _lib.call("emer_composite_rgb_bwd", _ptr(ts), _ptr(te), _ptr(sg), _ptr(c), _ptr(sk), _ptr(w), _ptr(stats), _ptr(gr), _ptr(go),
                      _ptr(gd), _ptr(gw), _ptr(gT), R, S, _ptr(dsig), _ptr(drgb), _ptr(dsky), _stream(sg))
        if c is not None and ctx.needs_input_grad[3] and drgb is None:
            drgb = torch.zeros_like(c)
        return None, None, (dsig if ctx.needs_input_grad[2] else None), drgb, dsky


# one launch each way for the static model's rendering (EMER_FUSE_COMPOSITE=0: the three kernels of rounds 1-3)
FUSE_COMPOSITE = os.environ.get("EMER_FUSE_COMPOSITE", "1") != "0"


def composite_rgb(t_starts: Tensor, t_ends: Tensor, sigma: Tensor, rgb: Optional[Tensor], rgb_sky: Optional[Tensor]):
    _check_cuda(t_starts, t_ends, sigma)
    return _CompositeRgbFn.apply(t_starts, t_ends, sigma, rgb, rgb_sky)


class _AccumulateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights: Tensor, values: Optional[Tensor]):
        w = _f32c(weights)
        R, S = w.shape
        v = _opt(values)
        C = 1 if v is None else v.shape[-1]
        with torch.cuda.device(w.device):
            out = _empty(w, R, C)
            _lib.call("emer_accumulate_fwd", _ptr(w), _ptr(v), R, S, C, _ptr(out), _stream(w))
        ctx.save_for_backward(w, v)
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):
        w, v = ctx.saved_tensors
        R, S = w.shape
        C = 1 if v is None else v.shape[-1]
        g = _f32c(dout)
        need_w, need_v = ctx.needs_input_grad[0], (v is not None and ctx.needs_input_grad[1])
        with torch.cuda.device(w.device):
            dw = torch.empty_like(w) if need_w else None
            dv = torch.empty_like(v) if need_v else None
            if need_w or need_v:
                _lib.call("emer_accumulate_bwd", _ptr(w), _ptr(v), _ptr(g), R, S, C, _ptr(dw), _ptr(dv), _stream(w))
        return dw, dv


def accumulate_along_rays(weights: Tensor, values: Optional[Tensor] = None) -> Tensor:
    """nerfacc.accumulate_along_rays on dense (R,S)/(R,S,C) tensors -> (R,C)."""
    _check_cuda(weights, values)
    return _AccumulateFn.apply(weights, values)


class _RayEpilogueFn(torch.autograd.Function):
    """(opacity [R,1], depth [R,1], median_depth [R,1], rgb [R,3] | None) from the scan kernel's per-ray sums
    (render_utils.py:102-122,217-226)."""

    @staticmethod
    def forward(ctx, stats: Tensor, acc_rgb: Optional[Tensor], rgb_sky: Optional[Tensor]):
        ctx.set_materialize_grads(False)
        st = _f32c(stats)
        R = st.shape[0]
        ar, sk = _opt(acc_rgb), _opt(rgb_sky)
        with torch.cuda.device(st.device):
            opa, dep, med = (_empty(st, R, 1) for _ in range(3))
            rgb = _empty(st, R, 3) if ar is not None else None
            _lib.call("emer_ray_epilogue_fwd", _ptr(st), _ptr(ar), _ptr(sk), R, _ptr(opa), _ptr(dep), _ptr(med), _ptr(rgb), _stream(st))
        ctx.save_for_backward(st, sk)
        ctx.has_rgb = ar is not None
        ctx.mark_non_differentiable(med)
        return opa, dep, med, rgb

    @staticmethod
    def backward(ctx, do, dd, dm, drgb):
        st, sk = ctx.saved_tensors
        R = st.shape[0]
        if do is None and dd is None and drgb is None:
            return None, None, None
        go, gd, gr = _opt(do), _opt(dd), _opt(drgb)
        with torch.cuda.device(st.device):
            dst = _empty(st, R, 4)
            dsk = _empty(st, R, 3) if (sk is not None and gr is not None) else None
            _lib.call("emer_ray_epilogue_bwd", _ptr(st), _ptr(sk), _ptr(go), _ptr(gd), _ptr(gr), R, _ptr(dst), _ptr(dsk), _stream(st))
        return dst, (gr if ctx.has_rgb else None), dsk


def ray_epilogue(stats: Tensor, acc_rgb: Optional[Tensor] = None, rgb_sky: Optional[Tensor] = None):
    """Per-ray tail of `rendering`: opacity = clamp(sum w, 1e-6, 1), depth = sum(w t) / opacity, median depth, and
    rgb = acc_rgb + rgb_sky * (1 - opacity).  Returns (opacity, depth, median_depth, rgb)."""
    _check_cuda(stats, acc_rgb, rgb_sky)
    return _RayEpilogueFn.apply(stats, acc_rgb, rgb_sky)


class _PixelLossFn(torch.autograd.Function):
    """w_rgb * mse(rgb, pixels) + w_sky * bce(opacity, 1 - sky_mask) (loss/base.py:83-185), one launch each way."""

    @staticmethod
    def forward(ctx, rgb: Tensor, opacity: Optional[Tensor], pixels: Tensor, sky_mask: Optional[Tensor], w_rgb: float, w_sky: float,
                grad_scale: float = 1.0):
        r, px = _f32c(rgb).view(-1, 3), _f32c(pixels).view(-1, 3)
        R = r.shape[0]
        op = None if opacity is None else _f32c(opacity).view(-1)
        sm = None if sky_mask is None else _f32c(sky_mask).view(-1)
        with torch.cuda.device(r.device):
            rays = torch.empty((R,), device=r.device, dtype=torch.float32)
            loss = torch.empty((), device=r.device, dtype=torch.float32)
            _lib.call("emer_pixel_loss_fwd", _ptr(r), _ptr(px), _ptr(op), _ptr(sm), R, float(w_rgb), float(w_sky), _ptr(rays), _ptr(loss),
                      _stream(r))
        ctx.save_for_backward(r, px, op, sm)
        ctx.w, ctx.shapes = (float(w_rgb) * float(grad_scale), float(w_sky) * float(grad_scale)), (rgb.shape, None if opacity is None else opacity.shape)
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        r, px, op, sm = ctx.saved_tensors
        R = r.shape[0]
        need_o = op is not None and ctx.needs_input_grad[1]
        gc = _f32c(g).reshape(1)
        with torch.cuda.device(r.device):
            dr = torch.empty_like(r) if ctx.needs_input_grad[0] else None
            do = torch.empty_like(op) if need_o else None
            _lib.call("emer_pixel_loss_bwd", _ptr(r), _ptr(px), _ptr(op), _ptr(sm), R, ctx.w[0], ctx.w[1], _ptr(gc), _ptr(dr), _ptr(do),
                      _stream(r))
        return (None if dr is None else dr.view(ctx.shapes[0])), (None if do is None else do.view(ctx.shapes[1])), None, None, None, None, None


def pixel_loss(rgb: Tensor, opacity: Optional[Tensor], pixels: Tensor, sky_mask: Optional[Tensor], w_rgb: float = 1.0,
               w_sky: float = 0.001, grad_scale: float = 1.0) -> Tensor:
    """rgb L2 + opacity-based sky BCE of a pixel-ray batch as one scalar (0-dim tensor).  ``grad_scale`` multiplies the
    GRADIENTS only (a trainer's loss scale folded into the backward kernel: the returned value stays the plain loss and
    no ``loss * scale`` launch, nor its backward, is needed)."""
    _check_cuda(rgb, opacity, pixels, sky_mask)
    return _PixelLossFn.apply(rgb, opacity, pixels, sky_mask, w_rgb, w_sky, grad_scale)


REG_MAX_BLOCKS = CONST["EMER_REG_MAX_BLOCKS"]


class _RegLossesFn(torch.autograd.Function):
    """base + the mean-type regularisers (dynamic-density / shadow sparsity, feature L2, flow cycle) as one launch each way."""

    @staticmethod
    def forward(ctx, base: Optional[Tensor], dyn: Optional[Tensor], shadow: Optional[Tensor], feat: Optional[Tensor], feat_gt: Optional[Tensor],
                ff: Optional[Tensor], fpb: Optional[Tensor], bf: Optional[Tensor], bpf: Optional[Tensor], coefs, grad_scale: float):
        c_dyn, c_shadow, c_feat, c_cycle = (float(c) for c in coefs)
        ts = [None if t is None else _f32c(t) for t in (dyn, shadow, feat, feat_gt, ff, fpb, bf, bpf)]
        dyn_c, sh_c, ft_c, gt_c, ff_c, fpb_c, bf_c, bpf_c = ts
        ref = next(t for t in ts if t is not None)
        if ft_c is not None:
            assert gt_c is not None and gt_c.numel() == ft_c.numel(), "feature loss: prediction / target size mismatch"
        if fpb_c is not None:
            assert all(t is not None and t.numel() == fpb_c.numel() for t in (ff_c, bf_c, bpf_c)), "flow cycle loss: size mismatch"
        n = lambda t: 0 if t is None else t.numel()
        bc = None if base is None else _f32c(base).reshape(1)
        with torch.cuda.device(ref.device):
            ws = torch.empty((REG_MAX_BLOCKS,), device=ref.device, dtype=torch.float32)
            loss = torch.empty((), device=ref.device, dtype=torch.float32)
            ctx.args = (n(dyn_c), c_dyn, n(sh_c), c_shadow, n(ft_c), c_feat, n(fpb_c), c_cycle)
            _lib.call("emer_reg_losses_fwd", _ptr(dyn_c), n(dyn_c), c_dyn, _ptr(sh_c), n(sh_c), c_shadow, _ptr(ft_c), _ptr(gt_c), n(ft_c), c_feat,
                      _ptr(ff_c), _ptr(fpb_c), _ptr(bf_c), _ptr(bpf_c), n(fpb_c), c_cycle, _ptr(bc), _ptr(ws), _ptr(loss), _stream(ref))
        # the sparsity terms' gradients are constants: only the tensors a gradient READS are saved
        ctx.save_for_backward(ft_c, gt_c, ff_c, fpb_c, bf_c, bpf_c)
        ctx.present = (dyn_c is not None, sh_c is not None)
        ctx.shapes = tuple(None if t is None else t.shape for t in (dyn, shadow, feat, fpb, bpf))
        ctx.grad_scale, ctx.dev = float(grad_scale), ref.device
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        ft_c, gt_c, ff_c, fpb_c, bf_c, bpf_c = ctx.saved_tensors
        n_dyn, c_dyn, n_sh, c_shadow, n_ft, c_feat, n_fl, c_cycle = ctx.args
        ni = ctx.needs_input_grad
        gc = _f32c(g).reshape(1)
        with torch.cuda.device(ctx.dev):
            new = lambda shape: torch.empty(shape, device=ctx.dev, dtype=torch.float32)
            d_dyn = new(ctx.shapes[0]) if ctx.present[0] and ni[1] else None
            d_sh = new(ctx.shapes[1]) if ctx.present[1] and ni[2] else None
            d_ft = new(ctx.shapes[2]) if ft_c is not None and ni[3] else None
            d_fpb = new(ctx.shapes[3]) if fpb_c is not None and ni[6] else None
            d_bpf = new(ctx.shapes[4]) if bpf_c is not None and ni[8] else None
            if any(t is not None for t in (d_dyn, d_sh, d_ft, d_fpb, d_bpf)):
                # absent-term pointers: the sparsity terms are described by their counts alone (gradient = constant)
                _lib.call("emer_reg_losses_bwd", _ptr(d_dyn), n_dyn if d_dyn is not None else 0, c_dyn, _ptr(d_sh), n_sh if d_sh is not None else 0,
                          c_shadow, _ptr(ft_c), _ptr(gt_c), n_ft, c_feat, _ptr(ff_c), _ptr(fpb_c), _ptr(bf_c), _ptr(bpf_c), n_fl, c_cycle,
                          _ptr(gc), ctx.grad_scale, _ptr(d_dyn), _ptr(d_sh), _ptr(d_ft), _ptr(d_fpb), _ptr(d_bpf), _stream(gc))
        gb = g if ni[0] else None
        return gb, d_dyn, d_sh, d_ft, None, None, d_fpb, None, d_bpf, None, None


class _RegLosses6Fn(torch.autograd.Function):
    """_RegLossesFn with the cycle term read from the flow MLP's own outputs: ``flow`` [N, 6] at the sample positions (constants, as the
    reference detaches them) and ``flow2`` [2 N, 6] at the two warped sets -- no slice copies forward, ONE gradient tensor backward
    (the four slices cost four contiguous copies, two zero fills, two copies and a cat per step)."""

    @staticmethod
    def forward(ctx, base: Optional[Tensor], dyn: Optional[Tensor], shadow: Optional[Tensor], feat: Optional[Tensor], feat_gt: Optional[Tensor],
                flow: Tensor, flow2: Tensor, coefs, grad_scale: float):
        c_dyn, c_shadow, c_feat, c_cycle = (float(c) for c in coefs)
        dyn_c, sh_c, ft_c, gt_c = (None if t is None else _f32c(t) for t in (dyn, shadow, feat, feat_gt))
        f6, f26 = _f32c(flow).view(-1, 6), _f32c(flow2).view(-1, 6)
        assert f26.shape[0] == 2 * f6.shape[0], "flow cycle loss: the warped evaluations must hold two rows per sample"
        if ft_c is not None:
            assert gt_c is not None and gt_c.numel() == ft_c.numel(), "feature loss: prediction / target size mismatch"
        n = lambda t: 0 if t is None else t.numel()
        bc = None if base is None else _f32c(base).reshape(1)
        dev = f6.device
        with torch.cuda.device(dev):
            ws = torch.empty((REG_MAX_BLOCKS,), device=dev, dtype=torch.float32)
            loss = torch.empty((), device=dev, dtype=torch.float32)
            ctx.args = (n(dyn_c), c_dyn, n(sh_c), c_shadow, n(ft_c), c_feat, f6.shape[0], c_cycle)
            _lib.call("emer_reg_losses_fwd6", _ptr(dyn_c), n(dyn_c), c_dyn, _ptr(sh_c), n(sh_c), c_shadow, _ptr(ft_c), _ptr(gt_c), n(ft_c), c_feat,
                      _ptr(f6), _ptr(f26), f6.shape[0], c_cycle, _ptr(bc), _ptr(ws), _ptr(loss), _stream(f6))
        ctx.save_for_backward(ft_c, gt_c, f6, f26)
        ctx.present = (dyn_c is not None, sh_c is not None)
        ctx.shapes = tuple(None if t is None else t.shape for t in (dyn, shadow, feat, flow2))
        ctx.grad_scale, ctx.dev = float(grad_scale), dev
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        ft_c, gt_c, f6, f26 = ctx.saved_tensors
        n_dyn, c_dyn, n_sh, c_shadow, n_ft, c_feat, n_rows, c_cycle = ctx.args
        ni = ctx.needs_input_grad
        gc = _f32c(g).reshape(1)
        with torch.cuda.device(ctx.dev):
            new = lambda shape: torch.empty(shape, device=ctx.dev, dtype=torch.float32)
            d_dyn = new(ctx.shapes[0]) if ctx.present[0] and ni[1] else None
            d_sh = new(ctx.shapes[1]) if ctx.present[1] and ni[2] else None
            d_ft = new(ctx.shapes[2]) if ft_c is not None and ni[3] else None
            d_f2 = new(ctx.shapes[3]) if ni[6] else None
            if any(t is not None for t in (d_dyn, d_sh, d_ft, d_f2)):
                _lib.call("emer_reg_losses_bwd6", _ptr(d_dyn), n_dyn if d_dyn is not None else 0, c_dyn, _ptr(d_sh), n_sh if d_sh is not None else 0,
                          c_shadow, _ptr(ft_c), _ptr(gt_c), n_ft, c_feat, _ptr(f6), _ptr(f26), n_rows, c_cycle, _ptr(gc), ctx.grad_scale,
                          _ptr(d_dyn), _ptr(d_sh), _ptr(d_ft), _ptr(d_f2), _stream(gc))
        gb = g if ni[0] else None
        return gb, d_dyn, d_sh, d_ft, None, None, d_f2, None, None


def reg_losses(base: Optional[Tensor] = None, dynamic_density: Optional[Tensor] = None, shadow_ratio: Optional[Tensor] = None,
               feat: Optional[Tensor] = None, feat_gt: Optional[Tensor] = None, forward_flow: Optional[Tensor] = None,
               forward_pred_backward_flow: Optional[Tensor] = None, backward_flow: Optional[Tensor] = None,
               backward_pred_forward_flow: Optional[Tensor] = None, c_dyn: float = 0.01, c_shadow: float = 0.01, c_feat: float = 0.5,
               c_cycle: float = 0.005, grad_scale: float = 1.0, flow_pair=None) -> Tensor:
    """``base + c_dyn mean(dynamic_density) + c_shadow mean(shadow_ratio) + c_feat mse(feat, feat_gt) + c_cycle mean((ff + fpb)^2 +
    (bf + bpf)^2)`` as a 0-dim tensor: loss/base.py:394-398 (sparsity), :83-146 (feature L2), train_emernerf.py:700-716 (cycle;
    forward_flow / backward_flow are constants, as the reference detaches them).  Absent terms are None.  ``grad_scale`` multiplies
    the regularisers' GRADIENTS only (``base`` passes its gradient through unscaled: its own kernel already folded the scale)."""
    if flow_pair is not None:
        # [r5] (flow at the samples [., 6], flow at the two warped sets [2 N, 6]): the four flow arguments are column blocks of this pair
        flow, flow2 = flow_pair
        _check_cuda(*[t for t in (base, dynamic_density, shadow_ratio, feat, feat_gt, flow, flow2) if t is not None])
        return _RegLosses6Fn.apply(base, dynamic_density, shadow_ratio, feat, feat_gt, flow.detach(), flow2, (c_dyn, c_shadow, c_feat, c_cycle), grad_scale)
    present = [t for t in (dynamic_density, shadow_ratio, feat, forward_pred_backward_flow) if t is not None]
    if not present:
        if base is None:
            raise ValueError("reg_losses: no term given")
        return base
    _check_cuda(*[t for t in (base, dynamic_density, shadow_ratio, feat, feat_gt, forward_flow, forward_pred_backward_flow, backward_flow,
                              backward_pred_forward_flow) if t is not None])
    return _RegLossesFn.apply(base, dynamic_density, shadow_ratio, feat, feat_gt, forward_flow, forward_pred_backward_flow, backward_flow,
                              backward_pred_forward_flow, (c_dyn, c_shadow, c_feat, c_cycle), grad_scale)


class _LidarLossFn(torch.autograd.Function):
    """w_depth * depth loss + w_sight * line-of-sight loss of a lidar-ray batch (train_emernerf.py:770-808)."""

    @staticmethod
    def forward(ctx, depth: Tensor, weights: Tensor, ranges: Tensor, t_vals: Tensor, epsilon: float, max_depth: float,
                w_depth: float, w_sight: float):
        dp, w, rg, tv = _f32c(depth).view(-1), _f32c(weights), _f32c(ranges).view(-1), _f32c(t_vals)
        R, S = w.shape
        with torch.cuda.device(w.device):
            ws = torch.empty((R + 2,), device=w.device, dtype=torch.float32)
            loss = torch.empty((), device=w.device, dtype=torch.float32)
            _lib.call("emer_lidar_loss", _ptr(dp), _ptr(rg), _ptr(w), _ptr(tv), R, S, float(epsilon), float(max_depth), float(w_depth),
                      float(w_sight), None, _ptr(ws), _ptr(loss), None, None, _stream(w))
        ctx.save_for_backward(dp, w, rg, tv)
        ctx.cfg, ctx.dshape = (float(epsilon), float(max_depth), float(w_depth), float(w_sight)), depth.shape
        return loss

    @staticmethod
    def backward(ctx, g: Tensor):
        dp, w, rg, tv = ctx.saved_tensors
        R, S = w.shape
        eps, md, wd, wsg = ctx.cfg
        gc = _f32c(g).reshape(1)
        with torch.cuda.device(w.device):
            ws = torch.empty((R + 2,), device=w.device, dtype=torch.float32)
            dd = torch.empty((R,), device=w.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
            _lib.call("emer_lidar_loss", _ptr(dp), _ptr(rg), _ptr(w), _ptr(tv), R, S, eps, md, wd, wsg, _ptr(gc), _ptr(ws), None, _ptr(dd),
                      _ptr(dw), _stream(w))
        return (None if dd is None else dd.view(ctx.dshape)), dw, None, None, None, None, None, None


def lidar_loss(depth: Tensor, weights: Tensor, lidar_ranges: Tensor, t_vals: Tensor, epsilon: float, max_depth: float = 80.0,
               w_depth: float = 1.0, w_sight: float = 0.1) -> Tensor:
    """Depth (loss/base.py:188-271, l2) + line-of-sight (loss/base.py:430-464) supervision as one scalar; gradients flow
    to the rendered depth [R,1] and the rendering weights [R,S].

    One divergence from the reference: a batch with NO valid ray (none with 0.01 < range < max_depth).  The reference's depth
    term is the mean of an empty tensor there, NaN (loss/base.py:60-72, 240-248); here the depth term is 0, its gradient is
    exact zeros and the valid count is never divided by, so the total stays finite and the line-of-sight term is unchanged.
    A batch with no ray of range > 0 has a line-of-sight term and weight gradients of exactly 0, as in the reference."""
    _check_cuda(depth, weights, lidar_ranges, t_vals)
    return _LidarLossFn.apply(depth, weights, lidar_ranges, t_vals, epsilon, max_depth, w_depth, w_sight)


# ---------------------------------------------------------------------------------- MLP heads
class _LinearFn(torch.autograd.Function):
    """act(x W^T + b) (+ optional density side output exp(pre[:,0] - 1))."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int, with_density: bool):
        ctx.set_materialize_grads(False)
        lead = x.shape[:-1]
        K = x.shape[-1]
        x2 = _f32c(x).view(-1, K)
        wc = _f32c(weight)
        bc = None if bias is None else _f32c(bias)
        M, N = x2.shape[0], wc.shape[0]
        with torch.cuda.device(x2.device):
            y = torch.empty((M, N), device=x2.device, dtype=torch.float32)
            aux = torch.empty((M,), device=x2.device, dtype=torch.float32) if with_density else None
            _lib.call("emer_linear_fwd", _ptr(x2), K, _ptr(wc), _ptr(bc), _ptr(y), N, M, N, K, act, _ptr(aux), _stream(x2))
        ctx.save_for_backward(x2, wc, y, aux)
        ctx.act, ctx.lead, ctx.has_bias = act, lead, bias is not None
        if with_density:
            return y.view(*lead, N), aux.view(*lead)
        return y.view(*lead, N)

    @staticmethod
    def backward(ctx, dy: Optional[Tensor], daux: Optional[Tensor] = None):
        x2, wc, y, aux = ctx.saved_tensors
        M, K = x2.shape
        N = wc.shape[0]
        if dy is None and daux is None:
            return None, None, None, None, None
        g = None if dy is None else _f32c(dy).view(M, N)
        ga = None if daux is None else _f32c(daux).view(M)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        with torch.cuda.device(x2.device):
            want_w = need_w or need_b
            n_ws = int(_lib.load().emer_linear_bwd_workspace(M, N, K)) if want_w else 0
            ws = torch.empty((n_ws,), device=x2.device, dtype=torch.float32) if want_w else None
            dx = torch.empty((M, K), device=x2.device, dtype=torch.float32) if need_x else None
            dw = torch.zeros((N, K), device=x2.device, dtype=torch.float32) if (need_w or need_b) else None
            db = torch.zeros((N,), device=x2.device, dtype=torch.float32) if need_b else None
            _lib.call("emer_linear_bwd", _ptr(g), N, _ptr(y), N, _ptr(x2), K, _ptr(wc), _ptr(ws), _ptr(dx), K, _ptr(dw),
                      _ptr(db), M, N, K, ctx.act, _ptr(ga), _ptr(aux), _stream(x2))
        return (dx.view(*ctx.lead, K) if need_x else None), (dw if need_w else None), db, None, None


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: Optional[str] = None) -> Tensor:
    """act(x @ weight.T + bias) on the fp32 matrix cores; act in {None,'relu','sigmoid','trunc_exp'}."""
    _check_cuda(x, weight, bias)
    return _LinearFn.apply(x, weight, bias, _ACTS[act], False)


def linear_with_density(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(x @ weight.T + bias, exp(pre[..., 0] - 1)): last base-MLP layer with the density activation
    of geometry feature 0 fused into the epilogue (radiance_field.py:28,315,422)."""
    _check_cuda(x, weight, bias)
    return _LinearFn.apply(x, weight, bias, ACT_NONE, True)


class _TruncExpFn(torch.autograd.Function):
    """density = exp(x[..., col] - 1) read off one column of a feature tensor."""

    @staticmethod
    def forward(ctx, feats: Tensor, col: int):
        f = feats.detach()
        assert f.dtype == torch.float32 and f.is_contiguous()
        C = f.shape[-1]
        n = f.numel() // C
        with torch.cuda.device(f.device):
            y = torch.empty(f.shape[:-1], device=f.device, dtype=torch.float32)
            src = f.view(-1)[col:]
            _lib.call("emer_trunc_exp_fwd", _ptr(src), C, _ptr(y), n, _stream(f))
        ctx.save_for_backward(y)
        ctx.col, ctx.shape = col, feats.shape
        return y

    @staticmethod
    def backward(ctx, dy: Tensor):
        (y,) = ctx.saved_tensors
        C = ctx.shape[-1]
        g = _f32c(dy)
        with torch.cuda.device(y.device):
            dx = torch.zeros(ctx.shape, device=y.device, dtype=torch.float32)
            dst = dx.view(-1)[ctx.col:]
            _lib.call("emer_trunc_exp_bwd", _ptr(g), _ptr(y), _ptr(dst), C, y.numel(), _stream(y))
        return dx, None


def trunc_exp_column(feats: Tensor, col: int = 0) -> Tensor:
    """trunc_exp(feats[..., col] - 1) (radiance_field.py:28,461)."""
    _check_cuda(feats)
    return _TruncExpFn.apply(feats.contiguous(), col)


class _Aggregate3Fn(torch.autograd.Function):
    """(cur + 0.5 fwd + 0.5 bwd) / 2 of a [3 N, C] batch laid out [current | forward-warped | backward-warped]
    (temporal_aggregation, radiance_field.py:553-620) -> [N, C]; one launch each way."""

    @staticmethod
    def forward(ctx, x3: Tensor):
        x = _f32c(x3)
        n3, C = x.shape
        assert n3 % 3 == 0 and (n3 // 3 * C) % 4 == 0
        with torch.cuda.device(x.device):
            out = torch.empty((n3 // 3, C), device=x.device, dtype=torch.float32)
            _lib.call("emer_aggregate3_fwd", _ptr(x), out.numel(), _ptr(out), _stream(x))
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        gc = _f32c(g)
        with torch.cuda.device(gc.device):
            dx = torch.empty((3 * gc.shape[0], gc.shape[1]), device=gc.device, dtype=torch.float32)
            _lib.call("emer_aggregate3_bwd", _ptr(gc), gc.numel(), _ptr(dx), _stream(gc))
        return dx


def aggregate3(x3: Tensor) -> Tensor:
    _check_cuda(x3)
    return _Aggregate3Fn.apply(x3)


class _Aggregate3DensityFn(torch.autograd.Function):
    """[r4] (aggregated features [N, C], density [N] = trunc_exp(features[:, 0] - 1)) of a [3 N, C] batch, one launch each way: the
    density's gradient joins column 0 inside the backward kernel (bitwise the sum autograd would form from the separate trunc_exp)."""

    @staticmethod
    def forward(ctx, x3: Tensor):
        ctx.set_materialize_grads(False)
        x = _f32c(x3)
        n3, C = x.shape
        assert n3 % 3 == 0 and C % 4 == 0
        with torch.cuda.device(x.device):
            out = torch.empty((n3 // 3, C), device=x.device, dtype=torch.float32)
            dens = torch.empty((n3 // 3,), device=x.device, dtype=torch.float32)
            _lib.call("emer_aggregate3_density_fwd", _ptr(x), n3 // 3, C, _ptr(out), _ptr(dens), _stream(x))
        ctx.save_for_backward(dens)
        ctx.C = C
        return out, dens

    @staticmethod
    def backward(ctx, g, gd):
        (dens,) = ctx.saved_tensors
        if g is None and gd is None:
            return None
        gc = None if g is None else _f32c(g)
        gdc = None if gd is None else _f32c(gd).reshape(-1)
        n = dens.shape[0]
        with torch.cuda.device(dens.device):
            dx = torch.empty((3 * n, ctx.C), device=dens.device, dtype=torch.float32)
            _lib.call("emer_aggregate3_density_bwd", _ptr(gc), _ptr(gdc), _ptr(dens), n, ctx.C, _ptr(dx), _stream(dens))
        return dx


def aggregate3_density(x3: Tensor):
    _check_cuda(x3)
    return _Aggregate3DensityFn.apply(x3)


def dir_encode(dirs: Tensor, max_deg: int = 4, remap: bool = True) -> Tensor:
    """SinusoidalEncoder(3, 0, max_deg); remap=True applies (dirs+1)/2 first (radiance_field.py:629; no grad)."""
    _check_cuda(dirs)
    d = _f32c(dirs).view(-1, 3)
    width = 3 if max_deg == 0 else 3 * (1 + 2 * (max_deg + 1))
    with torch.cuda.device(d.device):
        out = torch.empty((d.shape[0], width), device=d.device, dtype=torch.float32)
        _lib.call("emer_dir_encode", _ptr(d), _ptr(out), d.shape[0], max_deg, int(remap), _stream(d))
    return out.view(*dirs.shape[:-1], width)


def adam_step(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, lr: float, beta1: float, beta2: float,
              eps: float, weight_decay: float, grad_scale: float, step: int) -> None:
    """In-place torch.optim.Adam step on one flat fp32 buffer.  The kernel reads and writes ``params.numel()`` floats of all four
    tensors through raw pointers, so each must be fp32, contiguous, on ``params``' device and of that length."""
    _check_cuda(params, grads, exp_avg, exp_avg_sq)
    for name, t in (("params", params), ("grads", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t.dtype != torch.float32:
            raise _lib.EmerError(f"adam_step: {name} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise _lib.EmerError(f"adam_step: {name} must be contiguous")
        if t.device != params.device:
            raise _lib.EmerError(f"adam_step: {name} is on {t.device}, params on {params.device}")
        if t.numel() != params.numel():
            raise _lib.EmerError(f"adam_step: {name} has {t.numel()} elements, params {params.numel()}")
    with torch.cuda.device(params.device):
        _lib.call("emer_adam_step", _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), float(lr),
                  float(beta1), float(beta2), float(eps), float(weight_decay), float(grad_scale), int(step), _stream(params))


# ------------------------------------------------------------------ static / dynamic / shadow blend + accumulation
class _BlendAccumulateFn(torch.autograd.Function):
    """(acc_rgb [R,3], acc_shadow_sq [R,1] | None) of rendering's decomposed colour path (render_utils.py:125-175)."""

    @staticmethod
    def forward(ctx, weights, density, static_density, dynamic_density, static_rgb, dynamic_rgb, shadow_ratio):
        ctx.set_materialize_grads(False)
        w, sg, ss, sd = _f32c(weights), _f32c(density), _f32c(static_density), _f32c(dynamic_density)
        rs, rd = _f32c(static_rgb), _f32c(dynamic_rgb)
        sh = None if shadow_ratio is None else _f32c(shadow_ratio).reshape(w.shape)
        R, S = w.shape
        with torch.cuda.device(w.device):
            acc = torch.empty((R, 3), device=w.device, dtype=torch.float32)
            acs = torch.empty((R, 1), device=w.device, dtype=torch.float32) if sh is not None else None
            _lib.call("emer_blend_accumulate_fwd", _ptr(w), _ptr(sg), _ptr(ss), _ptr(sd), _ptr(rs), _ptr(rd), _ptr(sh), R, S, _ptr(acc),
                      _ptr(acs), _stream(w))
        ctx.save_for_backward(w, sg, ss, sd, rs, rd, sh)
        ctx.sh_shape = None if shadow_ratio is None else shadow_ratio.shape
        return acc, acs

    @staticmethod
    def backward(ctx, g_rgb, g_sh):
        w, sg, ss, sd, rs, rd, sh = ctx.saved_tensors
        R, S = w.shape
        if g_rgb is None and g_sh is None:
            return (None,) * 7
        gr = None if g_rgb is None else _f32c(g_rgb)
        gs = None if g_sh is None else _f32c(g_sh).view(-1)
        need = ctx.needs_input_grad
        with torch.cuda.device(w.device):
            mk = lambda t, on: torch.empty_like(t) if on else None  # noqa: E731
            dw, dsg, dss, dsd = mk(w, need[0]), mk(sg, need[1]), mk(ss, need[2]), mk(sd, need[3])
            drs, drd = mk(rs, need[4]), mk(rd, need[5])
            dsh = mk(sh, need[6]) if sh is not None else None
            _lib.call("emer_blend_accumulate_bwd", _ptr(w), _ptr(sg), _ptr(ss), _ptr(sd), _ptr(rs), _ptr(rd), _ptr(sh), _ptr(gr), _ptr(gs), R, S,
                      _ptr(dw), _ptr(dsg), _ptr(dss), _ptr(dsd), _ptr(drs), _ptr(drd), _ptr(dsh), _stream(w))
        return dw, dsg, dss, dsd, drs, drd, (None if dsh is None else dsh.view(ctx.sh_shape))


class _BlendAccumulateWideFn(torch.autograd.Function):
    """acc [R,C] of rendering's decomposed FEATURE path (render_utils.py:247-252), one launch each way."""

    @staticmethod
    def forward(ctx, weights, density, static_density, dynamic_density, static_feat, dynamic_feat):
        ctx.set_materialize_grads(False)
        w, sg, ss, sd = _f32c(weights), _f32c(density).reshape(weights.shape), _f32c(static_density).reshape(weights.shape), \
            _f32c(dynamic_density).reshape(weights.shape)
        fs, fd = _f32c(static_feat), _f32c(dynamic_feat)
        R, S = w.shape
        C = fs.shape[-1]
        with torch.cuda.device(w.device):
            acc = torch.empty((R, C), device=w.device, dtype=torch.float32)
            _lib.call("emer_blend_accumulate_wide_fwd", _ptr(w), _ptr(sg), _ptr(ss), _ptr(sd), _ptr(fs), _ptr(fd), R, S, C, _ptr(acc), _stream(w))
        ctx.save_for_backward(w, sg, ss, sd, fs, fd)
        ctx.shapes = (density.shape, static_density.shape, dynamic_density.shape)
        return acc

    @staticmethod
    def backward(ctx, g_acc):
        if g_acc is None:
            return (None,) * 6
        w, sg, ss, sd, fs, fd = ctx.saved_tensors
        R, S = w.shape
        C = fs.shape[-1]
        g = _f32c(g_acc)
        need = ctx.needs_input_grad
        with torch.cuda.device(w.device):
            mk = lambda t, on: torch.empty_like(t) if on else None  # noqa: E731
            dw, dsg, dss, dsd, dfs, dfd = mk(w, need[0]), mk(sg, need[1]), mk(ss, need[2]), mk(sd, need[3]), mk(fs, need[4]), mk(fd, need[5])
            _lib.call("emer_blend_accumulate_wide_bwd", _ptr(w), _ptr(sg), _ptr(ss), _ptr(sd), _ptr(fs), _ptr(fd), _ptr(g), R, S, C, _ptr(dw),
                      _ptr(dsg), _ptr(dss), _ptr(dsd), _ptr(dfs), _ptr(dfd), _stream(w))
        sh = ctx.shapes
        rs = lambda t, shape: None if t is None else t.view(shape)  # noqa: E731
        return dw, rs(dsg, sh[0]), rs(dss, sh[1]), rs(dsd, sh[2]), dfs, dfd


def blend_accumulate_wide(weights: Tensor, density: Tensor, static_density: Tensor, dynamic_density: Tensor, static_feat: Tensor,
                          dynamic_feat: Tensor) -> Tensor:
    """sum_s w (sigma_s / (sigma + 1e-6) feat_s + sigma_d / (sigma + 1e-6) feat_d) for [R,S,C] features -> [R,C]."""
    _check_cuda(weights, density, static_density, dynamic_density, static_feat, dynamic_feat)
    return _BlendAccumulateWideFn.apply(weights, density, static_density, dynamic_density, static_feat, dynamic_feat)


def blend_accumulate(weights: Tensor, density: Tensor, static_density: Tensor, dynamic_density: Tensor, static_rgb: Tensor,
                     dynamic_rgb: Tensor, shadow_ratio: Optional[Tensor] = None):
    """sum_s w (sigma_s / (sigma + 1e-6) rgb_s (1 - shadow) + sigma_d / (sigma + 1e-6) rgb_d) and sum_s w shadow^2."""
    _check_cuda(weights, density, static_density, dynamic_density, static_rgb, dynamic_rgb, shadow_ratio)
    return _BlendAccumulateFn.apply(weights, density, static_density, dynamic_density, static_rgb, dynamic_rgb, shadow_ratio)


# ------------------------------------------------------------------------------------ evaluation metrics
def _metric_out(out: Optional[Tensor], like: Tensor) -> Tensor:
    if out is None:
        return torch.empty(3, dtype=torch.float64, device=like.device)
    if out.dtype != torch.float64 or out.numel() != 3 or not out.is_contiguous() or out.device != like.device:
        raise _lib.EmerError("metric output slot: 3 contiguous float64 elements on the images' device")
    return out


def _row_mask(mask: Optional[Tensor], rows: int) -> Optional[Tensor]:
    """Any-dtype mask with ``rows`` elements -> contiguous fp32 whose nonzero entries mark the masked rows."""
    if mask is None:
        return None
    if mask.numel() != rows:
        raise _lib.EmerError(f"mask has {mask.numel()} elements, expected {rows}")
    m = mask.detach().reshape(rows)
    return (m if m.dtype == torch.float32 else (m != 0).to(torch.float32)).contiguous()


def ssim(pred: Tensor, gt: Tensor, mask: Optional[Tensor] = None, out: Optional[Tensor] = None, full: bool = False):
    """SSIM of two [H, W, C] (or [H, W]) fp32 images, exactly as skimage.metrics.structural_similarity(pred, gt,
    data_range=1.0, channel_axis=-1) computes it (emer_ssim).  Writes the device scalars (ssim, masked_sum, masked_count)
    into ``out`` (3 contiguous float64 elements, e.g. a row slice of a caller tensor; allocated when None) without a host
    sync: masked_sum is the sum of the uncropped S map over the pixels x channels where ``mask`` ([H, W] or [H, W, 1], any
    dtype) is nonzero and masked_count their number, so masked_sum / masked_count is
    ``structural_similarity(..., full=True)[1][mask].mean()``.  Returns ``out``, or ``(out, S map [H, W, C])`` when ``full``.
    H < 7 or W < 7 raises, as in scikit-image."""
    _check_cuda(pred, gt, mask, out)
    if pred.shape != gt.shape or pred.dim() not in (2, 3):
        raise _lib.EmerError(f"ssim: need two [H, W, C] images of one shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    H, W = pred.shape[:2]
    C = pred.shape[2] if pred.dim() == 3 else 1
    x, y = _f32c(pred), _f32c(gt)
    m = _row_mask(mask, H * W)
    res = _metric_out(out, x)
    smap = torch.empty_like(x) if full else None
    with torch.cuda.device(x.device):
        ws = torch.empty(max(int(_lib.load().emer_ssim_workspace(H, W)), 1), dtype=torch.float64, device=x.device)
        _lib.call("emer_ssim", _ptr(x), _ptr(y), _ptr(m), H, W, C, _ptr(smap), _ptr(ws), _ptr(res), _stream(x))
    return (res, smap) if full else res


def sq_err_sums(pred: Tensor, target: Tensor, mask: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """(sum of (pred - target)^2, the same over the rows whose ``mask`` entry is nonzero, the number of such rows) in float64
    on the device (emer_sq_err_sums), for pred / target of shape [..., cols] fp32 and a mask with one entry per row (any
    dtype).  Written into ``out`` (3 contiguous float64 elements; allocated when None) without a host sync: mse =
    sum / (rows * cols), masked mse = masked_sum / (n_rows * cols)."""
    _check_cuda(pred, target, mask, out)
    if pred.shape != target.shape or pred.dim() < 1:
        raise _lib.EmerError(f"sq_err_sums: shapes differ: {tuple(pred.shape)} vs {tuple(target.shape)}")
    cols = pred.shape[-1]
    rows = pred.numel() // max(cols, 1)
    p, t = _f32c(pred), _f32c(target)
    m = _row_mask(mask, rows)
    res = _metric_out(out, p)
    with torch.cuda.device(p.device):
        ws = torch.empty(max(int(_lib.load().emer_sq_err_sums_workspace(rows, cols)), 1), dtype=torch.float64, device=p.device)
        _lib.call("emer_sq_err_sums", _ptr(p), _ptr(t), _ptr(m), rows, cols, _ptr(ws), _ptr(res), _stream(p))
    return res


# ------------------------------------------------------------------------------------ order statistics (radix select)
SELECT_JOBS_MAX = CONST["EMER_SELECT_JOBS_MAX"]
SELECT_SOURCES_MAX = CONST["EMER_SELECT_SOURCES_MAX"]                # distinct columns of one call
SELECT_PER_SOURCE_MAX = CONST["EMER_SELECT_PER_SOURCE_MAX"]          # distinct ranks / percentiles per column (a quantile takes two)
SELECT_ROWS_MAX = CONST["EMER_SELECT_ROWS_MAX"]
SELECT_VECTOR_ROWS = 1024     # rows that one workgroup takes per step on the 16-byte-load path (256 on the scalar path)
SELECT_MAX_BLOCKS = 1024      # beyond it the workgroups stride over the rows
_SEL_ORDER, _SEL_QUANTILE, _SEL_WPERCENT = CONST["EMER_SELECT_ORDER"], CONST["EMER_SELECT_QUANTILE"], CONST["EMER_SELECT_WPERCENT"]
_SelectJob = STRUCT["emer_select_job"]


def _select(src: Tensor, n: int, stride: int, radius: bool, weights: Optional[Tensor], jobs, out_dtype) -> Tensor:
    """``jobs``: a list of ``(column, output, param)`` over the contiguous fp32 ``src`` ([n * stride] elements) -> one value per job
    (emer_select).  Requests beyond what one call takes (``SELECT_*_MAX``) are split into several calls."""
    if not 1 <= n <= SELECT_ROWS_MAX:
        raise _lib.EmerError(f"order statistics need 1 <= n < 2^31 rows, got {n}")
    out = torch.empty(len(jobs), dtype=out_dtype, device=src.device)
    item = out.element_size()
    calls, cur, cols = [], [], {}
    for i in sorted(range(len(jobs)), key=lambda k: jobs[k][0]):      # column by column: a call reads the rows once for all of them
        col, output, param = jobs[i]
        need = 2 if output == _SEL_QUANTILE else 1
        if len(cur) == SELECT_JOBS_MAX or cols.get(col, 0) + need > SELECT_PER_SOURCE_MAX or (col not in cols and len(cols) == SELECT_SOURCES_MAX):
            calls.append(cur)
            cur, cols = [], {}
        cols[col] = cols.get(col, 0) + need
        cur.append((i, col, output, param))
    calls.append(cur)
    lib = _lib.load()
    with torch.cuda.device(src.device):
        ws = torch.empty(int(lib.emer_select_workspace_bytes(SELECT_JOBS_MAX)), dtype=torch.uint8, device=src.device)
        for part in calls:
            arr = (_SelectJob * len(part))()
            for k, (i, col, output, param) in enumerate(part):
                arr[k] = _SelectJob(int(col), output, float(param), out.data_ptr() + i * item)
            _lib.call("emer_select", _ptr(src), CONST["EMER_SELECT_RADIUS" if radius else "EMER_SELECT_COLUMNS"], stride, _ptr(weights), arr, len(part), n, _ptr(ws), _stream(src))
    return out


def _select_input(x: Tensor, dim: Optional[int]):
    """-> (contiguous fp32 [n, C] view or copy, n, C, the shape of the other dimensions)."""
    _check_cuda(x)
    if not x.dtype.is_floating_point or x.dtype == torch.float64:
        raise _lib.EmerError(f"order statistics are computed on fp32 keys: {x.dtype} is not supported")
    if dim is None:
        t = _f32c(x).reshape(-1, 1)
        rest = ()
    else:
        moved = x.detach().movedim(dim, 0)
        rest = tuple(moved.shape[1:])
        t = _f32c(moved).reshape(moved.shape[0], -1)
    return t, t.shape[0], t.shape[1], rest


def _as_list(v, what: str):
    if isinstance(v, Tensor):
        if v.dim() > 1:
            raise _lib.EmerError(f"{what}: a scalar or a 1-D sequence, got {tuple(v.shape)}")
        return v.dim() == 0, [float(a) for a in v.reshape(-1).tolist()]
    if isinstance(v, (int, float)):
        return True, [float(v)]
    return False, [float(a) for a in v]


def order_statistics(x: Tensor, ranks, dim: Optional[int] = None) -> Tensor:
    """The values of the 0-based ``ranks`` (an int or a sequence of ints) in ascending order of ``x`` along ``dim`` (``None``: of
    the flattened tensor), ``sort(x, dim)[0][rank]`` without the sort (emer_select: an exact radix select, any size below 2^31
    rows, the same bits from run to run).  NaN sorts last, -0 counts as +0 (a selected zero is +0).  Shape: ``[len(ranks), *rest]``,
    or ``rest`` for a scalar rank; dtype and device follow ``x``."""
    t, n, C, rest = _select_input(x, dim)
    scalar, rs = _as_list(ranks, "ranks")
    for r in rs:
        if r != int(r) or not 0 <= r < n:
            raise _lib.EmerError(f"order_statistics: rank {r} of {n} rows")
    out = _select(t, n, C, False, None, [(c, _SEL_ORDER, r) for r in rs for c in range(C)], torch.float32)
    out = out.reshape(len(rs), *rest).to(x.dtype)
    return out[0] if scalar else out


def quantile(x: Tensor, q, dim: Optional[int] = None, radius: bool = False) -> Tensor:
    """``torch.quantile(x, q, dim=dim, interpolation="linear")`` for a scalar or 1-D ``q`` (a float, a sequence or a tensor) without
    its sort and without its limit of 16 777 216 elements (emer_select): the rank ``float32(q) * float32(n - 1)`` in fp32, the two
    neighbouring order statistics and torch's lerp, NaN if the input holds one.  ``radius=True``: ``x`` is a [..., 3] flow and the
    quantile is taken over ``hypot(x[..., 0], x[..., 1])`` of all rows -- the expression the flow colour kernel evaluates -- without
    materialising it.  Shape as torch's: the reduced shape for a scalar ``q``, ``[len(q), ...]`` for a 1-D one."""
    scalar, qs = _as_list(q, "q")
    for v in qs:
        if not 0 <= v <= 1:
            raise _lib.EmerError(f"quantile() q values must be in the range [0, 1], got {v}")
    if radius:
        _check_cuda(x)
        t = _rows(x, 3, "quantile: flow")
        out = _select(t, t.shape[0], 3, True, None, [(0, _SEL_QUANTILE, v) for v in qs], torch.float32).to(x.dtype)
        return out[0] if scalar else out
    t, n, C, rest = _select_input(x, dim)
    out = _select(t, n, C, False, None, [(c, _SEL_QUANTILE, v) for v in qs for c in range(C)], torch.float32)
    out = out.reshape(len(qs), *rest).to(x.dtype)
    return out[0] if scalar else out


def weighted_percentile(x: Tensor, w: Tensor, ps) -> Tensor:
    """The reference's ``weighted_percentile(x, w, ps)`` (utils/visualization_tools.py:68-76) on the device, float64 [len(ps)]: the
    values of ``x`` in ascending order against their cumulative weights, read at ``ps / 100`` of the total by linear interpolation.
    Weights are clamped to [0, 1] and summed as integers of 2^-32, so the result is exact and the same from run to run (the
    reference sums in fp32, in the order of an unstable argsort).  Equal values form ONE node with their summed weight: for
    distinct values this is the reference in exact arithmetic; among tied values the reference's answer depends on the order its
    argsort happens to give them and may differ.  ``w=None`` weighs every element 1."""
    _check_cuda(x, w)
    scalar, pl = _as_list(ps, "ps")
    for p in pl:
        if not 0 <= p <= 100:
            raise _lib.EmerError(f"weighted_percentile: percentile {p} outside [0, 100]")
    t = _f32c(x).reshape(-1)
    wt = None if w is None else _per_row(w, t.numel(), "weighted_percentile: w")
    out = _select(t, t.numel(), 1, False, wt, [(0, _SEL_WPERCENT, p) for p in pl], torch.float64)
    return out[0] if scalar else out


# ------------------------------------------------------------------------------------ evaluation colours
COLOUR_JOBS_MAX = CONST["EMER_COLOUR_JOBS_MAX"]
_TRANSITIONS = (15, 6, 4, 11, 13, 6)
_WHEELS: dict = {}


def colour_wheel():
    """The cyclic flow colour wheel as a [56, 3] float32 numpy array (no GPU needed): the six hue transitions red -> yellow ->
    green -> cyan -> blue -> magenta -> red of lengths (15, 6, 4, 11, 13, 6), each ``linspace(from, to, length,
    endpoint=False)`` truncated to uint8, and the first row repeated at the end so that interpolation can wrap."""
    import numpy as np
    hues = [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255), (255, 0, 0)]
    wheel = np.zeros((sum(_TRANSITIONS), 3), dtype=np.uint8)
    start = 0
    for a, b, n in zip(hues[:-1], hues[1:], _TRANSITIONS):
        wheel[start:start + n] = np.linspace(np.array(a), np.array(b), n, endpoint=False)
        start += n
    return np.concatenate([wheel, wheel[:1]]).astype(np.float32)


def _wheel_on(device) -> Tensor:
    w = _WHEELS.get(device)
    if w is None:
        w = _WHEELS[device] = torch.from_numpy(colour_wheel()).to(device)
    return w


_FeatJob, _BlendJob, _FlowJob = STRUCT["emer_feature_colour_job"], STRUCT["emer_blend_over_job"], STRUCT["emer_flow_colour_job"]


def _rows(t: Tensor, cols: int, what: str) -> Tensor:
    """[..., cols] -> contiguous fp32 [rows, cols] (a contiguous fp32 input is a view: no copy)."""
    if t.dim() < 1 or t.shape[-1] != cols:
        raise _lib.EmerError(f"{what}: expected [..., {cols}], got {tuple(t.shape)}")
    return _f32c(t).reshape(-1, cols)


def _per_row(t: Tensor, rows: int, what: str) -> Tensor:
    if t.numel() != rows:
        raise _lib.EmerError(f"{what}: {t.numel()} elements for {rows} rows")
    return _f32c(t).reshape(rows)


def feature_colours_multi(jobs):
    """Several PCA-colour projections of one image as ONE launch (emer_feature_colours): ``jobs`` is a list of
    ``(feat [..., E], mat [E, 3], lo [3], hi [3], scale [...] | None)`` with one row count and one E; returns the list of
    ``clamp((feat @ mat - lo) / (hi - lo), 0, 1) [* scale]`` of shape [..., 3].  A true subtraction and division, torch's clamp
    (NaN stays NaN); a row's value does not depend on the other rows or members.  Not differentiable: call under no_grad."""
    if not 1 <= len(jobs) <= COLOUR_JOBS_MAX:
        raise _lib.EmerError(f"feature_colours: 1..{COLOUR_JOBS_MAX} jobs, got {len(jobs)}")
    E = jobs[0][0].shape[-1]
    arr, keep, outs = (_FeatJob * len(jobs))(), [], []
    n_rows = None
    for i, (feat, mat, lo, hi, scale) in enumerate(jobs):
        _check_cuda(feat, mat, lo, hi, scale)
        f = _rows(feat, E, "feature_colours: feat")
        if n_rows is None:
            n_rows = f.shape[0]
        if f.shape[0] != n_rows:
            raise _lib.EmerError("feature_colours: the jobs of one launch share the row count")
        if tuple(mat.shape) != (E, 3) or lo.numel() != 3 or hi.numel() != 3:
            raise _lib.EmerError(f"feature_colours: need mat [{E}, 3], lo [3], hi [3]; got {tuple(mat.shape)}, {tuple(lo.shape)}, {tuple(hi.shape)}")
        m, l, h = _f32c(mat).to(f.device), _f32c(lo).reshape(3).to(f.device), _f32c(hi).reshape(3).to(f.device)
        s = None if scale is None else _per_row(scale, n_rows, "feature_colours: scale")
        out = _empty(f, *feat.shape[:-1], 3)
        keep.append((f, m, l, h, s))
        outs.append(out)
        arr[i] = _FeatJob(f.data_ptr(), m.data_ptr(), l.data_ptr(), h.data_ptr(), None if s is None else s.data_ptr(), out.data_ptr())
    ref = keep[0][0]
    with torch.cuda.device(ref.device):
        _lib.call("emer_feature_colours", arr, len(jobs), n_rows, E, _stream(ref))
    return outs


def feature_colours(feat: Tensor, mat: Tensor, lo: Tensor, hi: Tensor, scale: Optional[Tensor] = None) -> Tensor:
    """``clamp((feat @ mat - lo) / (hi - lo), 0, 1) [* scale]``: [..., E] features to [..., 3] colours (see
    ``feature_colours_multi``)."""
    return feature_colours_multi([(feat, mat, lo, hi, scale)])[0]


def blend_over_multi(jobs):
    """Several over-blends of one image as ONE launch (emer_blend_over): ``jobs`` is a list of ``(a [..., 3], o [...], b [..., 3])``;
    returns the list of ``clip(a * o + b * (1 - o), 0, 1)``, every operation rounded on its own as numpy evaluates it."""
    if not 1 <= len(jobs) <= COLOUR_JOBS_MAX:
        raise _lib.EmerError(f"blend_over: 1..{COLOUR_JOBS_MAX} jobs, got {len(jobs)}")
    arr, keep, outs = (_BlendJob * len(jobs))(), [], []
    n_rows = None
    for i, (a, o, b) in enumerate(jobs):
        _check_cuda(a, o, b)
        x, y = _rows(a, 3, "blend_over: a"), _rows(b, 3, "blend_over: b")
        if n_rows is None:
            n_rows = x.shape[0]
        if x.shape[0] != n_rows or y.shape[0] != n_rows:
            raise _lib.EmerError("blend_over: a, b and the jobs of one launch share the row count")
        w = _per_row(o, n_rows, "blend_over: o")
        out = _empty(x, *a.shape[:-1], 3)
        keep.append((x, y, w))
        outs.append(out)
        arr[i] = _BlendJob(x.data_ptr(), w.data_ptr(), y.data_ptr(), out.data_ptr())
    ref = keep[0][0]
    with torch.cuda.device(ref.device):
        _lib.call("emer_blend_over", arr, len(jobs), n_rows, _stream(ref))
    return outs


def blend_over(a: Tensor, o: Tensor, b: Tensor) -> Tensor:
    """``clip(a * o + b * (1 - o), 0, 1)`` for [..., 3] ``a``, ``b`` and a per-row ``o`` (see ``blend_over_multi``)."""
    return blend_over_multi([(a, o, b)])[0]


AUTO = "auto"      # a colour range taken from the data itself, as the reference's defaults (its ``None``) do


def _is_auto(v) -> bool:
    return isinstance(v, str) and v == AUTO


def flow_colours_multi(flows, max_radius=1.0, background: str = "bright"):
    """The colour-wheel images of several [..., 3] flows of one shape as ONE launch (emer_flow_colours): the reference's
    ``scene_flow_to_rgb`` (hue from the angle of (x, y) by linear interpolation on the 55-step wheel, saturation ("bright") or
    value ("dark") from the radius / max_radius, the other axis beyond radius 1), in [0, 1].  ``max_radius="auto"`` is the
    reference's default rule (its ``flow_max_radius=None``): every flow is normalised by the 0.99 quantile of its own radius
    (``quantile(flow, 0.99, radius=True)``, 4 bytes read to the host per flow, then one colour launch per flow); a quantile of 0
    means no division.  ``max_radius=None`` itself keeps raising ``NotImplementedError``, as it always has here: the rule costs
    a pass over the flow and a host read, so it is asked for by name."""
    if background not in ("bright", "dark"):
        raise ValueError(f"background should be one the following: ('bright', 'dark'), not {background}.")
    if not 1 <= len(flows) <= COLOUR_JOBS_MAX:
        raise _lib.EmerError(f"flow_colours: 1..{COLOUR_JOBS_MAX} flows, got {len(flows)}")
    if max_radius is None:
        raise NotImplementedError('flow_colours: max_radius=None is not a radius; pass one, or max_radius="auto" for the reference\'s '
                                  "quantile rule")
    if _is_auto(max_radius):
        if any(f.shape != flows[0].shape for f in flows):
            raise _lib.EmerError("flow_colours: the flows of one launch share the row count")
        radii = [float(quantile(f, 0.99, radius=True)) for f in flows]
        # a NaN quantile (a flow that holds a NaN) fails the reference's ``flow_max_radius > 0`` like a zero: no division
        return [flow_colours_multi([f], r if r == r else 0.0, background)[0] for f, r in zip(flows, radii)]
    arr, keep, outs = (_FlowJob * len(flows))(), [], []
    n_rows = None
    for i, flow in enumerate(flows):
        _check_cuda(flow)
        f = _rows(flow, 3, "flow_colours: flow")
        if n_rows is None:
            n_rows = f.shape[0]
        if f.shape[0] != n_rows:
            raise _lib.EmerError("flow_colours: the flows of one launch share the row count")
        out = _empty(f, *flow.shape[:-1], 3)
        keep.append(f)
        outs.append(out)
        arr[i] = _FlowJob(f.data_ptr(), out.data_ptr())
    ref = keep[0]
    with torch.cuda.device(ref.device):
        _lib.call("emer_flow_colours", arr, len(flows), n_rows, _ptr(_wheel_on(ref.device)), float(max_radius),
                  1 if background == "dark" else 0, _stream(ref))
    return outs


def flow_colours(flow: Tensor, max_radius=1.0, background: str = "bright") -> Tensor:
    """``scene_flow_to_rgb(flow, flow_max_radius=max_radius, background=background)`` on the device (see ``flow_colours_multi``)."""
    return flow_colours_multi([flow], max_radius, background)[0]


# ------------------------------------------------------------------------------------ video frames (8-bit, merged)
FRAME_TILES_MAX = CONST["EMER_FRAME_TILES_MAX"]
TILE_KINDS = {k: CONST["EMER_TILE_" + k.upper()] for k in ("colour3", "grey1", "one_minus_grey1", "depth")}
_FrameTile = STRUCT["emer_frame_tile"]
_TURBO8: dict = {}


def turbo_table():
    """The 256 x 3 turbo colours as a float64 numpy array (no GPU needed): matplotlib's listed ``turbo`` map, kept as data in
    ``_turbo.py``."""
    import numpy as np
    from ._turbo import TURBO
    return np.array(TURBO, dtype=np.float64)


def turbo_table_8bit():
    """``uint8(255 * clip(table, 0, 1))`` in fp64: what the reference's 8-bit cast makes of a depth colour -- one of 256 fixed
    byte triples.  [256, 3] uint8 numpy array."""
    import numpy as np
    return (255 * np.clip(turbo_table(), 0, 1)).astype(np.uint8)


def _turbo8_on(device) -> Tensor:
    t = _TURBO8.get(device)
    if t is None:
        t = _TURBO8[device] = torch.from_numpy(turbo_table_8bit()).to(device)
    return t


def depth_range(lo=4.0, hi=120.0, depth: Optional[Tensor] = None, opacity: Optional[Tensor] = None) -> Tuple[float, float]:
    """``(min(lo', hi'), |hi' - lo'|)`` of the curved bounds ``lo' = -log(lo + 1e-6)``, ``hi' = -log(hi + 1e-6)`` in fp64: the two
    constants of the depth colouring (no GPU needed when both bounds are numbers).  A bound of ``"auto"`` is the reference's default
    (its ``None``; ``visualize_cmap``, utils/visualization_tools.py:111-118) and needs the image: with ``lo_auto, hi_auto =
    weighted_percentile(depth, opacity, [0.5, 99.5])`` (16 bytes read to the host), ``lo = lo or (lo_auto - eps32)`` and ``hi = hi
    or (hi_auto + eps32)`` -- as there, a given bound of 0 is replaced too.  A bound of ``None`` itself keeps raising
    ``NotImplementedError``, as it always has here: the rule costs five passes over the image and a host read, so it is asked
    for by name."""
    import numpy as np
    if lo is None or hi is None:
        raise NotImplementedError('depth colours: lo=None / hi=None are not bounds; pass both, or "auto" for the weighted-percentile '
                                  "bounds of the image (ops.depth_colours, ops.depth_range with depth and opacity)")
    if _is_auto(lo) or _is_auto(hi):
        if depth is None or opacity is None:
            raise ValueError('depth_range: a bound of "auto" is a weighted percentile of one image: pass its depth and opacity')
        lo_auto, hi_auto = weighted_percentile(depth, opacity, [0.5, 99.5]).tolist()
        eps = float(np.finfo(np.float32).eps)
        lo = (None if _is_auto(lo) else lo) or (lo_auto - eps)
        hi = (None if _is_auto(hi) else hi) or (hi_auto + eps)
    with np.errstate(all="ignore"):
        lo_c, hi_c = -np.log(np.float64(lo) + 1e-6), -np.log(np.float64(hi) + 1e-6)
    return float(np.minimum(lo_c, hi_c)), float(np.abs(hi_c - lo_c))


def compose_frame(tiles, H: int, W: int, rows: int, cams: int, fp64_scale: bool, lo=4.0, hi=120.0, out: Optional[Tensor] = None) -> Tensor:
    """One merged 8-bit video frame, uint8 [rows * H, cams * W, 3], from device images (emer_compose_frame: ONE launch per
    ``FRAME_TILES_MAX`` tiles).  ``tiles`` is a list of ``(kind, row, col, src, opacity | None)``: ``src`` fills the cell
    (row, col) of the frame; ``kind`` is "colour3" (src [H, W, 3]: ``uint8(255 * clip(x, 0, 1))``), "grey1" (src [H, W] on three
    channels), "one_minus_grey1" (``1 - src``) or "depth" (src and opacity [H, W]: the reference's ``depth_visualizer`` with
    the bounds ``lo``, ``hi`` -- ``-log(x + 1e-6)`` scaled to [0, 1] between the curved bounds, times the opacity, as a row of
    the turbo table).  ``fp64_scale``: the product with 255 in fp64, as in the reference's frames that hold a depth row.  A NaN
    colour is written as 0.  Sources may be views with a storage offset; anything that is not contiguous fp32 is copied.  Cells
    that no tile names are zero.  A pixel's bytes depend on its own inputs, the kind and the flag alone.  A bound of ``"auto"``
    is the weighted-percentile bound of the frame's ONE depth tile (``depth_range``); a launch has one range, so with any other
    number of depth tiles ``"auto"`` raises.  ``None`` raises as it always has.  ``out``: a contiguous uint8 device frame of that
    shape to write into; the cells that no tile names are then left as they are (``five_view_frame``)."""
    auto = (_is_auto(lo) or _is_auto(hi)) and lo is not None and hi is not None
    if auto and sum(1 for t in tiles if t[0] == "depth") != 1:
        raise NotImplementedError('compose_frame: a bound of "auto" is a weighted percentile of one depth image and a launch has one '
                                  "range: implemented for a frame with exactly one depth tile; pass both bounds otherwise")
    if not auto:
        dmin, dabs = depth_range(lo, hi)
    H, W, rows, cams = int(H), int(W), int(rows), int(cams)
    if not tiles:
        raise ValueError("compose_frame: no tiles")
    arr, keep, cells = (_FrameTile * len(tiles))(), [], set()
    for i, (kind, row, col, src, opacity) in enumerate(tiles):
        if kind not in TILE_KINDS:
            raise ValueError(f"compose_frame: tile {i}: kind should be one of {tuple(TILE_KINDS)}, not {kind!r}")
        _check_cuda(src, opacity)
        want = (H, W, 3) if kind == "colour3" else (H, W)
        if tuple(src.shape) != want:
            raise ValueError(f"compose_frame: tile {i} ({kind}): expected {want}, got {tuple(src.shape)}")
        if kind == "depth" and (opacity is None or tuple(opacity.shape) != want):
            raise ValueError(f"compose_frame: tile {i}: a depth tile needs an opacity of shape {want}")
        if not (0 <= row < rows and 0 <= col < cams):
            raise ValueError(f"compose_frame: tile {i}: cell ({row}, {col}) outside the {rows} x {cams} frame")
        s, o = _f32c(src), (_f32c(opacity) if kind == "depth" else None)
        keep.append((s, o))
        cells.add((int(row), int(col)))
        arr[i] = _FrameTile(s.data_ptr(), None if o is None else o.data_ptr(), TILE_KINDS[kind], int(row), int(col), 0)
    ref = keep[0][0]
    if auto:
        d, o = next(k for k, t in zip(keep, tiles) if t[0] == "depth")
        dmin, dabs = depth_range(lo, hi, d, o)
    shape = (rows * H, cams * W, 3)
    if out is None:
        out = (torch.empty if len(cells) == rows * cams else torch.zeros)(shape, dtype=torch.uint8, device=ref.device)
    else:
        _check_frame(out, shape, ref.device, "compose_frame")
    rng = (ctypes.c_double * 2)(dmin, dabs)
    with torch.cuda.device(ref.device):
        table = _turbo8_on(ref.device)
        for first in range(0, len(tiles), FRAME_TILES_MAX):
            n = min(FRAME_TILES_MAX, len(tiles) - first)
            part = ctypes.cast(ctypes.byref(arr, first * ctypes.sizeof(_FrameTile)), ctypes.c_void_p)
            _lib.call("emer_compose_frame", part, n, H, W, rows, cams, 1 if fp64_scale else 0, ctypes.cast(rng, ctypes.c_void_p), _ptr(table),
                      _ptr(out), _stream(ref))
    return out


def depth_colours(depth: Tensor, opacity: Tensor, lo=4.0, hi=120.0) -> Tensor:
    """The reference's ``depth_visualizer`` cut to 8 bits, uint8 [H, W, 3], of a [H, W] depth and opacity: a one-tile frame
    (see ``compose_frame``).  ``lo`` / ``hi`` of ``"auto"`` are the reference's defaults (its ``None``): the image's own weighted-percentile
    bounds (``depth_range``)."""
    if depth.dim() != 2:
        raise ValueError(f"depth_colours: expected a [H, W] depth, got {tuple(depth.shape)}")
    H, W = depth.shape
    return compose_frame([("depth", 0, 0, depth, opacity)], H, W, 1, 1, False, lo, hi)


def _check_frame(out: Tensor, shape, device, what: str) -> None:
    if not isinstance(out, Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: `out` is a contiguous uint8 frame of shape {tuple(shape)} on the tiles' device")


# ------------------------------------------------------------------------------------ the five-view resize (cubic-spline zoom)
_TURBO64: dict = {}


def _turbo64_on(device) -> Tensor:
    t = _TURBO64.get(device)
    if t is None:
        t = _TURBO64[device] = torch.from_numpy(turbo_table()).to(device).contiguous()
    return t


def five_view_rows(W: int) -> int:
    """``int(W * 0.46)``: the rows that a resized outer view of a five-camera frame keeps (utils/visualization_tools.py:41)."""
    return int(int(W) * 0.46)


def _zoom_launch(tiles, H: int, W: int, h_out: int, rows: int, cams: int, fp64_scale: bool, lo, hi, frame: Tensor, values: Optional[Tensor]):
    """emer_zoom_tiles on checked ``(kind, row, col, src, opacity | None)`` tiles: ONE launch per ``FRAME_TILES_MAX`` tiles."""
    if not 2 <= h_out <= H:
        raise ValueError(f"zoom: {h_out} output rows from images of {H} rows: the resized view keeps 2 <= h <= H rows "
                         "(h = int(W * 0.46) in a five-view frame)")
    dmin, dabs = depth_range(lo, hi)
    arr, keep = (_FrameTile * len(tiles))(), []
    for i, (kind, row, col, src, opacity) in enumerate(tiles):
        if kind not in TILE_KINDS:
            raise ValueError(f"zoom: tile {i}: kind should be one of {tuple(TILE_KINDS)}, not {kind!r}")
        _check_cuda(src, opacity)
        want = (H, W, 3) if kind == "colour3" else (H, W)
        if tuple(src.shape) != want:
            raise ValueError(f"zoom: tile {i} ({kind}): expected {want}, got {tuple(src.shape)}")
        if kind == "depth" and (opacity is None or tuple(opacity.shape) != want):
            raise ValueError(f"zoom: tile {i}: a depth tile needs an opacity of shape {want}")
        if not (0 <= row < rows and 0 <= col < cams):
            raise ValueError(f"zoom: tile {i}: cell ({row}, {col}) outside the {rows} x {cams} frame")
        s, o = _f32c(src), (_f32c(opacity) if kind == "depth" else None)
        keep.append((s, o))
        arr[i] = _FrameTile(s.data_ptr(), None if o is None else o.data_ptr(), TILE_KINDS[kind], int(row), int(col), 0)
    ref = keep[0][0]
    rng = (ctypes.c_double * 2)(dmin, dabs)
    with torch.cuda.device(ref.device):
        table = _turbo64_on(ref.device)
        for first in range(0, len(tiles), FRAME_TILES_MAX):
            n = min(FRAME_TILES_MAX, len(tiles) - first)
            part = ctypes.cast(ctypes.byref(arr, first * ctypes.sizeof(_FrameTile)), ctypes.c_void_p)
            _lib.call("emer_zoom_tiles", part, n, H, W, h_out, rows, cams, 1 if fp64_scale else 0, ctypes.cast(rng, ctypes.c_void_p), _ptr(table),
                      _ptr(frame), _ptr(None if values is None else values[first:first + n]), _stream(ref))


def zoom_rows(x: Tensor, h_out: int, kind: str = "colour3", opacity: Optional[Tensor] = None, lo=4.0, hi=120.0) -> Tensor:
    """The values of the reference's ``scipy.ndimage.zoom(img, [h_out / H, 1, 1])`` (order 3, mirror prefilter) of one tile, fp64
    [h_out, W, 3], before the rounding to the image's type and the clip (emer_zoom_tiles, csrc/frames.hip): ``x`` is the tile's
    source as ``compose_frame`` takes it -- [H, W, 3] for "colour3", [H, W] for "grey1", "one_minus_grey1" (``1 - x`` in fp32)
    and "depth" (with ``opacity``; the zoom then reads the fp64 colours of ``turbo_table()``).  Only the y axis is computed: along
    x and the channels the reference's zoom is the identity up to its fp64 noise.  ``ValueError`` unless 2 <= h_out <= H.  A
    non-finite value spoils its own column and channel (the reference: the whole view)."""
    H, W = int(x.shape[0]), int(x.shape[1])
    h_out = int(h_out)
    _check_cuda(x, opacity)
    values = torch.empty((1, max(h_out, 0), W, 3), dtype=torch.float64, device=x.device)
    frame = torch.empty((H, W, 3), dtype=torch.uint8, device=x.device)
    _zoom_launch([(kind, 0, 0, x, opacity)], H, W, h_out, 1, 1, False, lo, hi, frame, values)
    return values[0]


def five_view_frame(tiles, H: int, W: int, rows: int, fp64_scale: bool, lo=4.0, hi=120.0) -> Tensor:
    """``compose_frame`` for a frame of five views under the reference's ``resize_five_views``: the tiles of columns 1 to 3 are
    composed as they are, the tiles of columns 0 and 4 become a black cell whose bottom ``five_view_rows(W)`` rows hold the
    cubic-spline zoom of the view (``zoom_rows``), clipped and cut to 8 bits -- colour and mask tiles after rounding to fp32 and
    by ``fp64_scale``, depth tiles in fp64 throughout.  ONE ``compose_frame`` launch and ONE zoom launch into the same frame
    (per ``FRAME_TILES_MAX`` tiles).  ``ValueError`` when ``int(W * 0.46)`` exceeds H (where the reference fails) or is below 2."""
    H, W, rows = int(H), int(W), int(rows)
    if not tiles:
        raise ValueError("five_view_frame: no tiles")
    if any(not 0 <= t[2] < 5 for t in tiles):
        raise ValueError("five_view_frame: a frame of five views has the columns 0 to 4")
    outer = [t for t in tiles if t[2] in (0, 4)]
    inner = [t for t in tiles if t[2] not in (0, 4)]
    h = five_view_rows(W)
    if outer and not 2 <= h <= H:
        raise ValueError(f"five_view_frame: the outer views keep int({W} * 0.46) = {h} rows, which should lie in 2 .. H = {H}")
    ref = tiles[0][3]
    _check_cuda(ref)
    cells = {(int(t[1]), int(t[2])) for t in tiles}
    frame = (torch.empty if len(cells) == rows * 5 else torch.zeros)((rows * H, 5 * W, 3), dtype=torch.uint8, device=ref.device)
    if inner:
        compose_frame(inner, H, W, rows, 5, fp64_scale, lo, hi, out=frame)
    if outer:
        _zoom_launch(outer, H, W, h, rows, 5, fp64_scale, lo, hi, frame, None)
    return frame


# ------------------------------------------------------------------------------------ voxel lift (bit masks)
VOXEL_JOBS_MAX, VOXELS_MAX = CONST["EMER_VOXEL_JOBS_MAX"], CONST["EMER_VOXELS_MAX"]
MEAN_ARRAYS_MAX = CONST["EMER_MEAN_ARRAYS_MAX"]
BITS_ROW_COLS_MAX = CONST["EMER_BITS_ROW_COLS_MAX"]
_VoxelMarkJob = STRUCT["emer_voxel_mark_job"]


def bit_words(n_bits: int) -> int:
    """Words of a mask of ``n_bits`` bits (bit n: word n // 32, position n % 32)."""
    return (int(n_bits) + 31) // 32


def _bits(bits: Tensor, n_bits: int, what: str) -> Tensor:
    if bits.dtype != torch.int32 or bits.dim() != 1 or not bits.is_contiguous() or bits.numel() != bit_words(n_bits):
        raise _lib.EmerError(f"{what}: the mask of {n_bits} bits is a contiguous int32 tensor of {bit_words(n_bits)} words, got "
                             f"{bits.dtype} {tuple(bits.shape)}")
    return bits


def _triple(v, kind, what: str):
    """Three host numbers (a sequence or a CPU / device tensor of 3 elements) -> a tuple of python ints or floats."""
    vals = v.detach().reshape(-1).tolist() if isinstance(v, Tensor) else list(v)
    if len(vals) != 3:
        raise _lib.EmerError(f"{what}: expected 3 values, got {len(vals)}")
    return tuple(kind(x) for x in vals)


def _voxel_count(res, what: str) -> int:
    if any(r < 1 or r >= 1 << 24 for r in res) or res[0] * res[1] * res[2] > VOXELS_MAX:
        raise _lib.EmerError(f"{what}: resolution {res}: every axis in 1 .. 2^24 - 1 and at most 2^31 - 1 voxels")
    return res[0] * res[1] * res[2]


def voxel_mark(jobs) -> None:
    """Mark the voxels that hold the ray end points ``origins + viewdirs * depth`` (emer_voxel_mark): ``jobs`` is a list of
    ``(origins [..., 3], viewdirs [..., 3], depth [...], max_depth, aabb_min (3), voxel_size (3), res (3), bits)`` that share the
    ray count and run as ONE launch (the static and the dynamic grid of an image).  ``bits`` is the grid's int32 mask of
    ``bit_words(prod(res))`` words and is updated in place (clear it with ``zero_()``); ``max_depth`` drops the rays with
    ``depth >= max_depth`` (``inf``: none).  The arithmetic is the reference's fp32 chain (visualization_tools.py:546-567,
    datasets/utils.py:85-88), the conversion truncates toward zero."""
    if not 1 <= len(jobs) <= VOXEL_JOBS_MAX:
        raise _lib.EmerError(f"voxel_mark: 1..{VOXEL_JOBS_MAX} jobs, got {len(jobs)}")
    arr, keep = (_VoxelMarkJob * len(jobs))(), []
    n_rays = None
    for i, (origins, viewdirs, depth, max_depth, aabb_min, voxel_size, res, bits) in enumerate(jobs):
        _check_cuda(origins, viewdirs, depth, bits)
        o, d = _rows(origins, 3, "voxel_mark: origins"), _rows(viewdirs, 3, "voxel_mark: viewdirs")
        if n_rays is None:
            n_rays = o.shape[0]
        if o.shape[0] != n_rays or d.shape[0] != n_rays:
            raise _lib.EmerError("voxel_mark: origins, viewdirs and the jobs of one launch share the ray count")
        t = _per_row(depth, n_rays, "voxel_mark: depth")
        res3 = _triple(res, int, "voxel_mark: res")
        b = _bits(bits, _voxel_count(res3, "voxel_mark"), "voxel_mark")
        if not (o.device == d.device == t.device == b.device):
            raise _lib.EmerError("voxel_mark: the rays and the mask of a job live on one device")
        keep.append((o, d, t, b))
        arr[i] = _VoxelMarkJob(o.data_ptr(), d.data_ptr(), t.data_ptr(), b.data_ptr(), float(max_depth),
                               (ctypes.c_float * 3)(*_triple(aabb_min, float, "voxel_mark: aabb_min")),
                               (ctypes.c_float * 3)(*_triple(voxel_size, float, "voxel_mark: voxel_size")), (ctypes.c_int32 * 3)(*res3))
    ref = keep[0][3]
    with torch.cuda.device(ref.device):
        _lib.call("emer_voxel_mark", arr, len(jobs), n_rays, _stream(ref))


def _bit_offsets(bits: Tensor, n_bits: int):
    """(offsets, total): the per-workgroup exclusive offsets of a mask's set bits and their number -- the ONE host read of a
    compaction."""
    with torch.cuda.device(bits.device):
        offsets = torch.empty(int(_lib.load().emer_bits_offsets_size(n_bits)), dtype=torch.int64, device=bits.device)
        _lib.call("emer_bits_offsets", _ptr(bits), n_bits, _ptr(offsets), _stream(bits))
    return offsets, int(offsets[-1].item())


def bits_nonzero_voxels(bits: Tensor, res, aabb_min, voxel_size, want_indices: bool = False):
    """The set bits of a voxel mask in ascending order as world corners ``aabb_min + float(i) * voxel_size`` ([M, 3] fp32; with
    ``want_indices`` also the [M, 3] int32 voxel indices): ``voxel_coords_to_world_coords(torch.nonzero(grid))`` of the
    reference.  One host synchronisation (the count); an empty mask gives [0, 3] outputs."""
    _check_cuda(bits)
    res3 = _triple(res, int, "bits_nonzero_voxels: res")
    n_bits = _voxel_count(res3, "bits_nonzero_voxels")
    _bits(bits, n_bits, "bits_nonzero_voxels")
    amin, vs = _triple(aabb_min, float, "bits_nonzero_voxels: aabb_min"), _triple(voxel_size, float, "bits_nonzero_voxels: voxel_size")
    offsets, total = _bit_offsets(bits, n_bits)
    coords = torch.empty(total, 3, dtype=torch.float32, device=bits.device)
    indices = torch.empty(total, 3, dtype=torch.int32, device=bits.device) if want_indices else None
    with torch.cuda.device(bits.device):
        _lib.call("emer_bits_emit_voxels", _ptr(bits), _ptr(offsets), total, (ctypes.c_int32 * 3)(*res3), (ctypes.c_float * 3)(*amin),
                  (ctypes.c_float * 3)(*vs), _ptr(coords), _ptr(indices), _stream(bits))
    return (coords, indices) if want_indices else coords


def bits_select_rows(bits: Tensor, src: Tensor) -> Tensor:
    """``src[selector]`` for a [N, C] fp32 ``src`` (C <= 4; a [N] tensor counts as C = 1 and gives [M]) and the selector held as a
    mask of N bits: the rows whose bit is set, in ascending order.  One host synchronisation (the count)."""
    _check_cuda(bits, src)
    if src.dim() not in (1, 2) or src.dtype != torch.float32 or (src.dim() == 2 and not 1 <= src.shape[1] <= BITS_ROW_COLS_MAX):
        raise _lib.EmerError(f"bits_select_rows: src is fp32 [N] or [N, 1..{BITS_ROW_COLS_MAX}], got {src.dtype} {tuple(src.shape)}")
    if src.device != bits.device:
        raise _lib.EmerError("bits_select_rows: the mask and the rows live on one device")
    n, cols = src.shape[0], (src.shape[1] if src.dim() == 2 else 1)
    _bits(bits, n, "bits_select_rows")
    if n == 0:
        return src.detach().clone()
    s = _f32c(src)
    offsets, total = _bit_offsets(bits, n)
    out = torch.empty((total, cols) if src.dim() == 2 else (total,), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.call("emer_bits_emit_rows", _ptr(bits), n, _ptr(offsets), total, _ptr(s), cols, _ptr(out), _stream(s))
    return out


def mean_threshold_bits(densities, thr: float) -> Tensor:
    """The selector ``mean(stack(densities), 0) > thr`` of K fp32 arrays of one length N as a mask of N bits (int32 words):
    ``((d0 + d1) + ...) / K > thr`` with a sequential fp32 sum and one division; K = 1 is ``d0 > thr``.  NaN selects nothing."""
    if isinstance(densities, Tensor):
        densities = [densities]
    if not 1 <= len(densities) <= MEAN_ARRAYS_MAX:
        raise _lib.EmerError(f"mean_threshold_bits: 1..{MEAN_ARRAYS_MAX} arrays, got {len(densities)}")
    _check_cuda(*densities)
    n = densities[0].numel()
    ds = []
    for d in densities:
        if d.numel() != n or d.dtype != torch.float32 or d.device != densities[0].device:
            raise _lib.EmerError("mean_threshold_bits: the arrays are fp32, of one length and on one device")
        ds.append(_f32c(d).reshape(n))
    bits = torch.empty(bit_words(n), dtype=torch.int32, device=ds[0].device)
    ptrs = (ctypes.c_void_p * len(ds))(*[d.data_ptr() for d in ds])
    with torch.cuda.device(ds[0].device):
        _lib.call("emer_mean_threshold_bits", ptrs, len(ds), n, float(thr), _ptr(bits), _stream(ds[0]))
    return bits
