"""Fused MLP heads: seven autograd Functions over the register-resident kernels of csrc/mlp_fused.hip / csrc/rayinputs.hip (hidden
width 64: every shipped config) and the generic LDS-staged ``emer_mlp_chain`` / ``emer_wgrad_segmented`` of csrc/mlp.hip (any other
width that fits its 512-column row buffer and 160 KiB of LDS at four waves).  Heads beyond that (``*_supported``) run layer by layer
on ``emer_linear_*``, outside these Functions.  All are HIP; there is no torch fallback.
  * ``base_mlp``    -- Linear(K0,H) ReLU Linear(H,NG) + density trunc_exp(out[:,0]-1) on the LEVEL-MAJOR grid encoding
                       (radiance_field.py:74-80,89-96,315,422); ``neck``: the same at H = 64 with 64 / 128 outputs;
  * ``density_mlp`` -- proposal net Linear(K0,H) ReLU Linear(H,1) trunc_exp (radiance_field.py:808-812,836-840);
  * ``rgb_head``    -- mlp.MLP(3 layers, skip at layer 1) + sigmoid on [dir-PE | appearance emb | geo] (radiance_field.py:130-143,
                       622-658), the per-ray part kept per ray; ``skip_mlp3``: that MLP on plain rows, the per-ray sky head;
  * ``seq_mlp`` / ``seq_mlp_lm`` -- plain stacks (shadow / flow / feature heads): ``_RMlpFn`` at hidden width 64, else ``_SeqMLPFn``.
What the backward needs (post-ReLU activations) is written once by the forward and read once as relu' masks / wgrad operands, or
recomputed by a backward that carries its own weight gradients.

WHICH kernels run is decided ONCE, in ``forward``, by a pure function of the shapes, the module flags and the library's host-only
queries (``<head>_path``), and recorded as ``ctx.path``; ``backward`` dispatches on it and on what only backward time knows (``dout
is None``, ``needs_input_grad``, whether ray_jobs may defer).  Without a backward (need_grad False) no in-kernel weight gradient is
chosen and nothing is stored.  The paths, as forward | backward entry points ("wgrad": one ``emer_wgrad_segmented``):
  neck         fused           emer_neck_fwd | emer_neck_bwd_fused
               streamed        emer_neck_fwd (stores h) | emer_neck_bwd, 2-3 wgrad
               (a rider replaces the forward launch of either by emer_[ray_pre_fwd +] emer_field_fwd)
  density_mlp  fused           emer_neck_fwd | emer_density_bwd_fused
               neck_streamed   emer_neck_fwd (stores h) | emer_neck_bwd, 2 wgrad
               chain           emer_mlp_chain | emer_mlp_chain, 2 wgrad
  base_mlp     chain           emer_mlp_chain | emer_mlp_chain, 2 wgrad
  rgb_head     fused           emer_ray_pre_fwd, emer_rgb_head_fwd | emer_rgb_head_bwd_fused, per-ray tail
               recompute_a1a2  the same, a1 and a2 not stored | emer_rgb_head_bwd_recompute, per-ray tail
               recompute_a2    the same, a2 not stored | emer_rgb_head_bwd_recompute, per-ray tail
               w2_in_kernel    the same, both stored | emer_rgb_head_bwd (with dW2), 2 wgrad, per-ray tail
               streamed        the same, both stored | emer_rgb_head_bwd, 3 wgrad, per-ray tail
               chain           emer_mlp_chain | emer_mlp_chain, 3 wgrad, torch sum over the samples
               (per-ray tail: emer_ray_wgrad, emer_ray_pre_bwd, deferred to ray_jobs after the first three; forward parked by a rider)
  skip_mlp3    ray             emer_ray_pre_fwd, emer_ray_head_fwd | emer_ray_head_bwd, emer_ray_pre_bwd, emer_ray_wgrad (or all in ray_jobs)
               ray_streamed    the same forward | emer_ray_head_bwd, emer_ray_pre_bwd, 3 wgrad (more than 65536 rows)
               chain           emer_mlp_chain | emer_mlp_chain, 3 wgrad
  seq_mlp(_lm) fused           emer_rmlp_fwd | emer_rmlp_bwd_fused
               streamed        emer_rmlp_fwd (stores h1, h2) | emer_rmlp_bwd, wgrad per layer
               chain           emer_mlp_chain | emer_mlp_chain, wgrad per layer (``_SeqMLPFn``)
"""
from __future__ import annotations

import contextlib
import functools
import os
import ctypes
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib, ray_jobs
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TRUNC_EXP, CONST, STRUCT, _ng, _stream  # noqa: F401
from ._lib import _f32c as _c, _ptr as _p

MAX_LAYERS, MAX_SEGS = CONST["EMER_CHAIN_MAX_LAYERS"], CONST["EMER_CHAIN_MAX_SEGS"]
E15 = 3269017.3724721107

ChainSeg, ChainLayer, ChainDesc = STRUCT["emer_chain_seg"], STRUCT["emer_chain_layer"], STRUCT["emer_chain_desc"]
RayWgradJob = ray_jobs.WgradJob

# ---------------------------------------------------------------------------------- flags (read when a forward runs)
FUSED_WGRAD = True   # weight gradients inside the backward kernels where the library has them (emer_neck_bwd_fused); False: separate pass
FUSED_RMLP_WGRAD = os.environ.get("EMER_FUSE_RMLP_WGRAD", "1") != "0"  # ... of the plain 2- / 3-layer heads with <= 16 outputs (emer_rmlp_bwd_fused) [r5]
FUSED_RMLP_WIDE = os.environ.get("EMER_FUSE_RMLP_WIDE", "1") != "0"    # ... incl. the 64-wide feature heads (one wave per SIMD, 192 accumulator registers)
FUSED_RGB_WGRAD = os.environ.get("EMER_FUSE_RGB_WGRAD", "1") != "0"   # ... of the rgb head's layers 0 / 1 too (emer_rgb_head_bwd_fused) [r4]
# [r6] ... optionally with a1 / a2 recomputed in that kernel from geo and the per-ray pre-activations (emer_rgb_head_bwd_recompute): the
# forward stores no hidden activations (512 B / sample less written and kept alive until the backward, 512 B / sample less read); bitwise
# the saved-activation path's results.  EMER_RGB_RECOMPUTE = 0: both stored (default); 1: both recomputed; 2: a1 stored, a2 recomputed.
# Same-session A/B at the metric shape (profiles/r06_ab_rgb_recompute.txt): field_fwd 311 -> 212 / 236 us, backward 368 -> 504 / 484 us,
# step 2.365 -> 2.385 / 2.405 ms -- the recomputation's 168 / 120 matrix instructions per tile cost more in the one-wave-per-SIMD
# backward than the stores cost the four-waves-per-SIMD forward.  It stays as the MEMORY mode (-537 MB of saved activations per million
# samples), off by default.
RGB_RECOMPUTE = int(os.environ.get("EMER_RGB_RECOMPUTE", "0"))
SIDE_STREAM = None  # a torch.cuda.Stream: set by a trainer that joins it before reading gradients (see wgrad)


# ------------------------------------------------------------------- the path of each head (see the module docstring)
def neck_path(n_levels: int, n_feat: int, n_rows: int, n_out: int, need_grad: bool) -> str:
    """fused: the backward recomputes the hidden layer from enc, so the forward does not store it (268 MB at 1 M rows)."""
    ok = FUSED_WGRAD and need_grad and _lib.load().emer_neck_bwd_fused_workspace(n_levels, n_feat, n_rows, n_out) > 0
    return "fused" if ok else "streamed"


def density_mlp_path(n_levels: int, n_feat: int, n_rows: int, hidden: int, need_grad: bool) -> str:
    """fused: narrow inputs (the proposal networks), one backward kernel with the weight gradients, hidden layer recomputed."""
    if not neck_supported(n_levels, n_feat, hidden, 1):
        return "chain"
    ok = FUSED_WGRAD and need_grad and _lib.load().emer_density_bwd_fused_workspace(n_levels, n_feat, n_rows) > 0
    return "fused" if ok else "neck_streamed"


def rgb_head_path(n_rays: int, samples_per_ray: int, Kh: int, H: int, NG: int, C: int, geo_ld: int, geo_ptr: int, need_grad: bool) -> str:
    """geo_ld / geo_ptr: row pitch (floats) and address of the geometry features (the register-resident kernels read 16 bytes at once)."""
    if not (H == 64 and NG == 64 and C == 3 and Kh <= 64 and samples_per_ray % 16 == 0 and geo_ld % 4 == 0 and geo_ptr % 16 == 0):
        return "chain"
    if not (FUSED_WGRAD and need_grad):
        return "streamed"
    if not (FUSED_RGB_WGRAD and _lib.load().emer_rgb_head_bwd_fused_workspace(n_rays, samples_per_ray) > 0):
        return "w2_in_kernel"   # the output layer's weight gradient (3 x 64 + 3 numbers) rides along in emer_rgb_head_bwd
    return _RGB_FUSED[int(RGB_RECOMPUTE)]


_RGB_FUSED = ("fused", "recompute_a1a2", "recompute_a2")


def skip_mlp3_path(n_rows: int, K0: int, H: int, C: int, need_grad: bool = True) -> str:
    """ray: a few thousand rows -- two small launches each way and ONE for all weight gradients beat the chain kernel's set-up."""
    if not (H == 64 and K0 <= 64 and C <= 16):
        return "chain"
    return "ray" if n_rows <= 65536 else "ray_streamed"


def seq_mlp_path(weights, n_feat: int, n_rows: int, need_grad: bool, hidden_biases: bool = True) -> str:
    """Plain stack of these Linear weights on row-major (n_feat 0) or level-major input.  fused [r5]: at most 16 outputs (flow MLP,
    shadow head) and the three-layer feature heads -- ONE backward kernel recomputes the hidden layers from x (it needs their
    biases) with the weight gradients in registers; the forward stores no activations.  chain: no stack of those kernels."""
    n, k0, n_out = len(weights), int(weights[0].shape[1]), int(weights[-1].shape[0])
    ok = (FUSED_WGRAD and FUSED_RMLP_WGRAD and n in (2, 3) and (n_out <= 16 or FUSED_RMLP_WIDE) and need_grad and hidden_biases
          and _lib.load().emer_rmlp_bwd_fused_workspace(n, k0, int(n_feat), int(n_rows), n_out) > 0)
    return "fused" if ok else "streamed" if rmlp_supported(weights, k0, n_feat) else "chain"


def rgb_recompute(n_rays: int, samples_per_ray: int) -> int:
    """Hidden activations that the backward of an rgb head of this shape recomputes (not stored): 0 none, 1 a1 and a2, 2 a2 only."""
    path = rgb_head_path(n_rays, samples_per_ray, 64, 64, 64, 3, 64, 0, True)
    return _RGB_FUSED.index(path) if path in _RGB_FUSED else 0


def rmlp_bwd_fused_supported(weights, k0: int, n_feat: int, n_rows: int) -> bool:
    """True when the backward of this stack runs as emer_rmlp_bwd_fused (weight gradients in the kernel, hidden layers recomputed)."""
    return int(k0) == weights[0].shape[1] and seq_mlp_path(weights, n_feat, n_rows, True) == "fused"


def _launch(name: str, ref: Tensor, *args) -> None:
    """One library call on the device of ``ref`` and on its current stream (every entry point's last argument)."""
    with torch.cuda.device(ref.device):
        _lib.call(name, *args, _stream(ref))


def _new(ref, *shape) -> Tensor:
    """Uninitialised fp32 tensor on the device of ``ref`` (a tensor or a device)."""
    return torch.empty(shape, device=getattr(ref, "device", ref), dtype=torch.float32)


def ray_wgrad(jobs, ref: Tensor) -> None:
    """Weight gradients of per-ray layers in ONE launch.  jobs: [(dy [M, n], [(x [M, >= width], width, dst_col), ...], dw, dbias | None)]
    -- dw[:, dst_col : dst_col + width] += dy^T x and dbias += colsum(dy), accumulated into the given tensors."""
    arr = (RayWgradJob * len(jobs))()
    M = jobs[0][0].shape[0]
    for a, (dy, blocks, dw, db) in zip(arr, jobs):
        assert dy.shape[0] == M and dy.stride(1) == 1 and dw.stride(1) == 1 and 1 <= len(blocks) <= 2
        a.dy, a.ld_dy, a.n, a.n_segs = dy.data_ptr(), dy.stride(0), dy.shape[1], len(blocks)
        a.dw, a.ld_dw, a.dbias = dw.data_ptr(), dw.stride(0), (None if db is None else db.data_ptr())
        for i, (x, width, dst) in enumerate(blocks):
            assert x.shape[0] == M and x.stride(1) == 1
            a.x[i], a.ld_x[i], a.width[i], a.dst_col[i] = x.data_ptr(), x.stride(0), width, dst
    _launch("emer_ray_wgrad", ref, arr, len(jobs), M)


def seg(t: Tensor, col: int, width: int, ld: Optional[int] = None, row_div: int = 1, dst_col: Optional[int] = None) -> ChainSeg:
    """Row-major segment: value(row, c) = t[(row // row_div), c].  dst_col (wgrad only): where the segment's gradient
    columns land in the output matrix (default: its own position in the virtual concatenation)."""
    s = ChainSeg(ptr=_p(t), ld=ld if ld is not None else t.stride(-2), n_total=0, fix_a=None, fix_b=None, col=col,
                 width=width, row_div=row_div, mode=0, f=1, dst_col=col if dst_col is None else dst_col)
    s._t = t  # keeps the tensor reachable (side-stream bookkeeping in wgrad)
    return s


def seg_lm(t: Tensor, col: int) -> ChainSeg:
    """Level-major grid encoding [L, N, F] as L*F columns."""
    L, N, F = t.shape
    s = ChainSeg(ptr=_p(t), ld=0, n_total=N, fix_a=None, fix_b=None, col=col, width=L * F, row_div=1, mode=1, f=F, dst_col=col)
    s._t = t
    return s


def layer(w: Tensor, bias: Optional[Tensor], in_col: int, out_col: int, act: int = ACT_NONE, transposed: bool = False,
          n_slice: Optional[Tuple[int, int]] = None, mask: Optional[Tensor] = None, store: Optional[Tensor] = None,
          store_cols: Optional[Tuple[int, int]] = None, store_lm: bool = False, store_exp0: Optional[Tensor] = None,
          accumulate: bool = False) -> ChainLayer:
    """w is a torch Linear weight [out, in].  transposed=True uses W^T (dgrad): output index runs over `in`.
    n_slice=(a, b) restricts the chain layer's outputs to [a, b) of that output index."""
    out_f, in_f = w.shape
    if not transposed:
        K, n_tot, sn, sk = in_f, out_f, w.stride(0), w.stride(1)
    else:
        K, n_tot, sn, sk = out_f, in_f, w.stride(1), w.stride(0)
    a, b = n_slice if n_slice is not None else (0, n_tot)
    ptr = w.data_ptr() + 4 * a * sn
    N = b - a
    L = ChainLayer(w=ptr, w_sn=sn, w_sk=sk, bias=None if bias is None else bias.data_ptr() + 4 * a, mask=_p(mask),
                   mask_ld=0 if mask is None else mask.stride(0), store=None, store_ld=0, store_ntotal=0,
                   store_exp0=_p(store_exp0), in_col=in_col, K=K, out_col=out_col, N=N, act=act, accumulate=int(accumulate),
                   store_col=0, store_n=0, store_mode=0, store_f=1)
    if store is not None:
        L.store = store.data_ptr()
        c0, c1 = store_cols if store_cols is not None else (0, N)
        L.store_col, L.store_n = c0, c1 - c0
        if store_lm:
            Lv, Nt, F = store.shape
            L.store_mode, L.store_f, L.store_ntotal = 1, F, Nt
            assert Lv * F == L.store_n
        else:
            L.store_ld = store.stride(0)
            assert store.shape[1] >= L.store_n
    return L


def run_chain(segs, layers, buf_cols: int, n_rows: int, ref: Tensor) -> None:
    d = ChainDesc()
    for i, s in enumerate(segs):
        d.segs[i] = s
    for i, l in enumerate(layers):
        # the kernel finishes one group of 64 output columns (GEMM over the whole K, then the epilogue's writes) before the next:
        # only the LAST group of a layer may write over the layer's own input
        if l.N > 64 and l.in_col < l.out_col + 64 * ((l.N - 1) // 64) and l.out_col < l.in_col + l.K:
            raise ValueError(f"chain layer {i}: output columns {l.out_col}..{l.out_col + l.N} written before the layer's last column "
                             f"group overlap its input {l.in_col}..{l.in_col + l.K}")
        d.layers[i] = l
    d.n_segs, d.n_layers, d.buf_cols = len(segs), len(layers), buf_cols
    _launch("emer_mlp_chain", ref, ctypes.byref(d), n_rows)


def wgrad(dpre: Tensor, segs, k_total: int, want_bias: bool = True, col0: Optional[Tensor] = None,
          out_w: Optional[Tensor] = None, out_b: Optional[Tensor] = None):
    """dW [N,K], db [N] for dpre [M,N] against the (virtually concatenated) segments.  col0 [M] replaces dpre[:, 0].
    out_w / out_b: ACCUMULATE into these instead of returning fresh tensors (out_w [N, >= K] with unit column stride;
    segment s lands at columns dst_col_s..).  Returns (dW or None, db or None)."""
    M, N = dpre.shape
    dev = dpre.device
    # Weight gradients that go straight into gradient sinks have no consumer inside the backward pass, so they can run
    # on a SIDE STREAM, concurrently with the data-gradient chain that continues on the main stream (neck backward,
    # grid backward: VALU/LDS-bound kernels that leave HBM idle, while these kernels are HBM-bound).  The trainer joins
    # the side stream before it touches the gradients (Trainer.train_step).
    side = SIDE_STREAM if (out_w is not None and (out_b is not None or not want_bias)) else None
    with torch.cuda.device(dev):
        if side is not None:
            main = torch.cuda.current_stream(dev)
            side.wait_stream(main)  # operands were produced on the main stream
            for t in [dpre, col0] + [getattr(sg, "_t", None) for sg in segs]:
                if t is not None:
                    t.record_stream(side)  # the caching allocator must not recycle them while the side stream reads
            ctx = torch.cuda.stream(side)
        else:
            ctx = contextlib.nullcontext()
        with ctx:
            n_ws = int(_lib.load().emer_linear_bwd_workspace(M, N, k_total))
            ws = torch.empty((n_ws,), device=dev, dtype=torch.float32)
            need_b = want_bias and out_b is None
            if out_w is None or need_b:
                buf = torch.zeros((N * (k_total if out_w is None else 0) + (N if need_b else 0),), device=dev, dtype=torch.float32)  # one fill
            dw = buf[:N * k_total].view(N, k_total) if out_w is None else None
            db = (buf[-N:] if need_b else None)
            tw = dw if out_w is None else out_w
            tb = out_b if out_b is not None else db
            assert tw.stride(1) == 1 and tw.dtype == torch.float32 and (tb is None or tb.is_contiguous())
            arr = (ChainSeg * MAX_SEGS)()
            for i, sg in enumerate(segs):
                arr[i] = sg
            _lib.call("emer_wgrad_segmented", _p(dpre), dpre.stride(0), _p(col0), arr, len(segs), _p(ws), _p(tw), tw.stride(0),
                      _p(tb) if want_bias else None, M, N, k_total, _stream(dpre))
    return dw, db


def join_side_stream() -> None:
    """Make the current stream wait for the weight-gradient side streams (no-op when unused)."""
    if SIDE_STREAM is not None:
        torch.cuda.current_stream().wait_stream(SIDE_STREAM)


def _sink(p) -> Optional[Tensor]:
    """The tensor a parameter's gradient may be accumulated into directly: its existing fp32 ``.grad`` with unit
    column stride.  This is what autograd's AccumulateGrad would do after the backward (``grad += dW``), fused into
    the weight-gradient reduction -- it saves a zero-fill and an add launch per parameter.  Opt-in and SCOPED
    (``with grad_sinks():`` around a forward+backward): parameter hooks are bypassed, so only a trainer that owns its
    gradient buffers enables it, and only for its own step.  Parameters that do not require grad never get a sink."""
    if not _USE_GRAD_SINKS:
        return None
    if not getattr(p, "requires_grad", False):
        return None
    g = getattr(p, "grad", None)
    if g is None or g.dtype != torch.float32 or not g.is_cuda or g.stride(-1) != 1:
        return None
    return g


_USE_GRAD_SINKS = False


@contextlib.contextmanager
def grad_sinks(enabled: bool = True):
    """Enable direct accumulation into ``.grad`` for the heads whose FORWARD runs inside this block (the decision is
    recorded per autograd node at forward time, so the matching backward may run inside or outside the block)."""
    global _USE_GRAD_SINKS
    prev, _USE_GRAD_SINKS = _USE_GRAD_SINKS, bool(enabled)
    try:
        yield
    finally:
        _USE_GRAD_SINKS = prev
        join_side_stream()   # (launches the block moved to the auxiliary stream are ordered before whatever follows it)


def _target(sink: Optional[Tensor], shape, dev):
    """(tensor to accumulate into, value to hand back to autograd): the parameter's .grad (-> None) or fresh zeros."""
    if sink is not None:
        return sink, None
    t = torch.zeros(shape, device=dev, dtype=torch.float32)
    return t, t


def _wb_shapes(Ws, need_b=None):
    """Shapes of (w0, b0, w1, b1, ...) for Linear weights Ws; None for a bias that takes no gradient (need_b[i] False)."""
    return [s for i, W in enumerate(Ws) for s in (tuple(W.shape), (W.shape[0],) if need_b is None or need_b[i] else None)]


def _targets(sinks, shapes, dev, last_layer_first: bool = False):
    """_target of all parameters (w0, b0, w1, b1, ...) of a head -> ([accumulate into], [hand to autograd]); shape None: (None, None).
    The zero fills are launched layer by layer, from the last layer if asked."""
    n = len(shapes)
    order = range(n) if not last_layer_first else [i + j for i in range(n - 2, -1, -2) for j in (0, 1)]
    tgt, ret = [None] * n, [None] * n
    for i in order:
        if shapes[i] is not None:
            tgt[i], ret[i] = _target(sinks[i], shapes[i], dev)
    return tgt, ret


def _split_wb(wb):
    """(w0, b0, w1, b1, ...) -> contiguous fp32 [weights], [biases or None]."""
    return [_c(w) for w in wb[0::2]], [None if b is None else _c(b) for b in wb[1::2]]


def _stack_shape(X: Tensor, level_major: bool):
    """(L, F, rows, K0) of a stack's input: level-major [L, rows, F], or row-major [rows, K0] (L = F = 0)."""
    if level_major:
        L, N, F = X.shape
        return L, F, N, L * F
    return 0, 0, X.shape[0], X.shape[1]


def _stack_wgrads(dpre, operands, Ws, sinks, need_b, dev):
    """Streamed weight gradients of a plain stack: dpre[i] against the segments operands[i] -> [dw0, db0, dw1, ...] for autograd."""
    grads = []
    for i, W in enumerate(Ws):
        tw, rw = _target(sinks[2 * i], tuple(W.shape), dev)
        tb, rb = _target(sinks[2 * i + 1], (W.shape[0],), dev) if need_b[i] else (None, None)
        wgrad(dpre[i], operands[i], W.shape[1], want_bias=need_b[i], out_w=tw, out_b=tb)
        grads += [rw, rb]
    return grads


def _ray_pre_fwd(x: Tensor, W0, B0, W1, B1, ref: Tensor) -> Tensor:
    """rb [rows, 2 H]: the share of x in the pre-activations of layers 0 | 1 of a skip head (x W0[:, :K]^T + b0 | x W1[:, H : H + K]^T + b1)."""
    n, K = x.shape
    H = W0.shape[0]
    rb = _new(ref, n, 2 * H)
    _launch("emer_ray_pre_fwd", ref, _p(x), x.stride(0), n, K, H, _p(W0), W0.stride(0), _p(B0), _p(W1[:, H:]), W1.stride(0), _p(B1),
            _p(rb), 2 * H)
    return rb


def _ray_pre_bwd(s0: Tensor, s1: Tensor, W0, W1, K: int, ref: Tensor) -> Tensor:
    """dx [rows, K] = s0 W0[:, :K] + s1 W1[:, H : H + K] for the gradients s0 / s1 [rows, H] of those pre-activations."""
    n, H = s0.shape
    dx = _new(ref, n, K)
    _launch("emer_ray_pre_bwd", ref, _p(s0), _p(s1), H, n, K, H, _p(W0), W0.stride(0), _p(W1[:, H:]), W1.stride(0), _p(dx), K)
    return dx


def _r4(x: int) -> int:
    return (x + 3) // 4 * 4


# ------------------------------------------------------------------------- row-buffer layouts of the chain heads
def _ru(x: int, m: int) -> int:
    return -(-x // m) * m


def chain_fits(buf_cols: int, kn) -> bool:
    """emer_mlp_chain's launch conditions for a descriptor with ``buf_cols`` row-buffer columns and layers kn = [(K, N), ...]:
    at most 512 columns, and the zero-padded weights plus the 16-row buffers of the MINIMUM four waves inside 160 KiB of LDS
    (chain_lds_plan / emer_mlp_chain of csrc/mlp.hip)."""
    w = sum(_ru(N, 16) * (_ru(K, 8) + 2) + _ru(N, 16) for K, N in kn)
    P = _ru(buf_cols + 8, 4) + 2
    return 4 <= buf_cols <= 512 and (_ru(w, 4) + 4 * 16 * P) * 4 <= 160 * 1024


def _skip_cols(H: int, K0: int, C: int):
    """Forward columns of the 3-layer skip heads: [A1 | x] from column 0 exactly like torch.cat([x_hidden, input]) of mlp.py:42,
    then A2, then the output.  A layer of at most 64 outputs is ONE column group of the kernel: every input column has been
    consumed by the MFMAs before its epilogue writes, so A2 may overwrite A1 in place (a smaller row buffer buys more waves per
    CU).  A wider layer runs group after group over the whole K, and group 1 would read an A1 whose first 64 columns already
    hold A2: it gets columns of its own.  Returns (c_x, c_a2, c_o, buf_cols)."""
    c_x = _r4(H)
    c_e = c_x + _r4(K0)
    c_a2 = 0 if c_x <= 64 else c_e
    c_o = c_e if c_a2 == 0 else c_e + c_x
    return c_x, c_a2, c_o, c_o + _r4(C)


def base_mlp_chain_shapes(K0: int, H: int, NG: int):
    """[(buf_cols, [(K, N) per layer])] of base_mlp's forward and backward chains."""
    return [(_r4(K0) + _r4(H) + NG, [(K0, H), (H, NG)]), (_r4(NG) + _r4(H) + K0, [(NG, H), (H, K0)])]


def density_mlp_chain_shapes(K0: int, H: int):
    return [(_r4(K0) + _ru(H, 8) + 4, [(K0, H), (H, 1)]), (4 + _r4(H) + K0, [(1, H), (H, K0)])]


def rgb_head_chain_shapes(H: int, Kh: int, NG: int, C: int):
    K0 = Kh + NG
    return [(_skip_cols(H, K0, C)[3], [(K0, H), (H + K0, H), (H, C)]),
            (_r4(C) + 2 * H + K0, [(C, H), (H, H), (H, K0), (H, Kh), (H, NG)])]


def skip_mlp3_chain_shapes(H: int, K0: int, C: int):
    return [(_skip_cols(H, K0, C)[3], [(K0, H), (H + K0, H), (H, C)]),
            (_r4(C) + 2 * H + _r4(K0), [(C, H), (H, H), (H, K0), (H, K0)])]


def _all_fit(shapes) -> bool:
    return all(chain_fits(b, kn) for b, kn in shapes)


@functools.lru_cache(maxsize=None)
def base_mlp_supported(K0: int, H: int, NG: int) -> bool:
    """The forward and the backward chain of base_mlp fit the chain kernel (otherwise base_mlp runs layer by layer)."""
    return _all_fit(base_mlp_chain_shapes(K0, H, NG))


@functools.lru_cache(maxsize=None)
def density_mlp_supported(K0: int, H: int) -> bool:
    return _all_fit(density_mlp_chain_shapes(K0, H))


@functools.lru_cache(maxsize=None)
def rgb_head_supported(H: int, Kh: int, NG: int, C: int) -> bool:
    return H % 4 == 0 and _all_fit(rgb_head_chain_shapes(H, Kh, NG, C))


@functools.lru_cache(maxsize=None)
def skip_mlp3_supported(H: int, K0: int, C: int) -> bool:
    return H % 4 == 0 and _all_fit(skip_mlp3_chain_shapes(H, K0, C))


def _skip3_layers(x: Tensor, w0, b0, w1, b1, w2, b2, final_act: int) -> Tensor:
    """The 3-layer skip MLP layer by layer on emer_linear_* (ops.linear): heads too wide for one chain launch."""
    from . import ops
    h = ops.linear(x, w0, b0, "relu")
    h = ops.linear(torch.cat([h, x], dim=-1), w1, b1, "relu")
    return ops.linear(h, w2, b2, "sigmoid" if final_act == ACT_SIGMOID else None)


def _skip_chain_fwd(parts, W0, B0, W1, B1, W2, B2, final_act: int, N: int, ref: Tensor):
    """The 3-layer skip head on the chain kernel -> (a1, a2, out).  parts: [(tensor, width, seg keywords)], the column blocks of
    the input; the row buffer is [A1 | input], A2 in place over A1 when H <= 64 (see _skip_cols)."""
    H, C = W0.shape[0], W2.shape[0]
    c_x, c_a2, c_o, cols = _skip_cols(H, sum(w for _, w, _ in parts), C)
    a1, a2, out = _new(ref, N, H), _new(ref, N, H), _new(ref, N, C)
    segs, c = [], c_x
    for t, w, kw in parts:
        segs.append(seg(t, c, w, **kw))
        c += w
    run_chain(segs,
              [layer(W0, B0, c_x, 0, ACT_RELU, store=a1),
               layer(W1, B1, 0, c_a2, ACT_RELU, store=a2),
               layer(W2, B2, c_a2, c_o, final_act, store=out)],
              cols, N, ref)
    return a1, a2, out


def _skip_chain_bwd(dpre2: Tensor, W0, W1, W2, a1, a2, tail, in_cols: int, ref: Tensor):
    """Data gradients of that head from the caller's dpre2 -> (dpre1, dpre0).  tail: [(a, b, store)], the input-gradient columns
    [a, b) -- W0's share accumulated onto W1's -- and where they are stored; in_cols: buffer columns kept for the input gradient."""
    N, C = dpre2.shape
    H, K0 = W0.shape
    dpre1, dpre0 = _new(ref, N, H), _new(ref, N, H)
    c1 = _r4(C)                 # dA2 -> dPre1
    cx = c1 + H                 # d[A1 | input]; dA1 -> dPre0 in place
    run_chain([seg(dpre2, 0, C)],
              [layer(W2, None, 0, c1, transposed=True, mask=a2, store=dpre1),
               layer(W1, None, c1, cx, transposed=True, n_slice=(0, H), mask=a1, store=dpre0),
               layer(W1, None, c1, cx + H, transposed=True, n_slice=(H, H + K0))]
              + [layer(W0, None, cx, cx + H + a, transposed=True, n_slice=(a, b), accumulate=True, store=st) for a, b, st in tail],
              cx + H + in_cols, N, ref)
    return dpre1, dpre0


def _lm2_chain_bwd(s0: ChainSeg, c_h: int, W0, W1, h, enc):
    """Data gradients of Linear-ReLU-Linear on a level-major encoding, on the chain kernel -> (dpre0, denc).  s0: the segment of the
    output layer's gradient at column 0, c_h columns wide in the row buffer."""
    L, N, F = enc.shape
    H = W0.shape[0]
    dpre0, denc = _new(enc, N, H), _new(enc, L, N, F)
    c_e = c_h + _r4(H)
    run_chain([s0],
              [layer(W1, None, 0, c_h, transposed=True, mask=h, store=dpre0),
               layer(W0, None, c_h, c_e, transposed=True, store=denc, store_lm=True)],
              c_e + L * F, N, enc)
    return dpre0, denc


# ------------------------------------------------------------------------------------------ base MLP
class _BaseMLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor):
        ctx.set_materialize_grads(False)
        enc, W0, B0, W1, B1 = _c(enc_lm), _c(w0), _c(b0), _c(w1), _c(b1)
        L, N, F = enc.shape
        K0, H, NG = L * F, W0.shape[0], W1.shape[0]
        ctx.path = "chain"
        h1, g, dens = _new(enc, N, H), _new(enc, N, NG), _new(enc, N)
        c_h = _r4(K0)
        c_g = c_h + _r4(H)
        run_chain([seg_lm(enc, 0)],
                  [layer(W0, B0, 0, c_h, ACT_RELU, store=h1), layer(W1, B1, c_h, c_g, ACT_NONE, store=g, store_exp0=dens)],
                  c_g + NG, N, enc)
        ctx.save_for_backward(enc, W0, W1, h1, dens)
        return g, dens

    @staticmethod
    def backward(ctx, dg: Optional[Tensor], ddens: Optional[Tensor]):
        enc, W0, W1, h1, dens = ctx.saved_tensors
        L, N, F = enc.shape
        K0, H, NG = L * F, W0.shape[0], W1.shape[0]
        if dg is None and ddens is None:
            return None, None, None, None, None
        dgt = torch.zeros((N, NG), device=enc.device, dtype=torch.float32) if dg is None else _c(dg)
        # trunc_exp backward (nerf_utils.py:69-72) is merged into geometry feature 0 INSIDE the kernels:
        # column 0 += ddens * min(dens, e^15) while the operand is staged (no 268 MB clone / strided add)
        fa = None if ddens is None else _c(ddens)
        fb = None if ddens is None else dens
        s0 = seg(dgt, 0, NG)
        s0.fix_a, s0.fix_b = _p(fa), _p(fb)
        dpre0, denc = _lm2_chain_bwd(s0, _r4(NG), W0, W1, h1, enc)
        col0 = None if fa is None else dgt[:, 0] + fa * dens.clamp(max=E15)
        dw1, db1 = wgrad(dgt, [seg(h1, 0, H)], H, col0=col0)
        dw0, db0 = wgrad(dpre0, [seg_lm(enc, 0)], K0)
        return denc, dw0, db0, dw1, db1


def base_mlp(enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor) -> Tuple[Tensor, Tensor]:
    """(feats [N, NG], density [N]) from the level-major grid encoding [L, N, F]."""
    L, _, F = enc_lm.shape
    if not base_mlp_supported(L * F, w0.shape[0], w1.shape[0]):
        from . import ops   # too wide for one chain launch: layer by layer on emer_linear_*
        return ops.linear_with_density(ops.linear(ops.lm_to_rm(enc_lm), w0, b0, "relu"), w1, b1)
    return _BaseMLPFn.apply(*_ng(enc_lm, w0, b0, w1, b1))


# ------------------------------------------------------------------------------- neck (register-resident)
def neck_supported(n_levels: int, n_feat: int, hidden: int, n_out: int) -> bool:
    return bool(_lib.load().emer_neck_supported(n_levels, n_feat, hidden, n_out))


class RgbRider:
    """A colour query that rides along in the neck's forward launch (emer_field_fwd): the neck Function computes the rgb head's
    activations and output together with the geometry features and parks them here; the rgb head Function that is called
    next WITH THOSE geometry features picks them up instead of launching its own forward.  The autograd graph (neck node ->
    rgb node) and both backward passes are exactly those of the separate calls."""

    def __init__(self, hray: Tensor, samples_per_ray: int, params, keep: bool):
        self.hray, self.S, self.params, self.keep = hray, int(samples_per_ray), tuple(params), bool(keep)
        self.geo_ptr = None
        self.rb = self.a1 = self.a2 = self.out = None   # rb: the per-ray pre-activations [R, 128] of layers 0 | 1
        self.geo = self.versions = None                 # while parked: the geometry features and _versions of the query's tensors

    def usable(self, L: int, F: int, N: int, n_out: int) -> bool:
        w0, _, w1, _, w2, _ = self.params
        R, Kh = self.hray.shape
        return bool(n_out == 64 and self.S % 16 == 0 and R * self.S == N and Kh <= 64 and w0.shape == (64, Kh + 64)
                    and w1.shape == (64, 128 + Kh) and w2.shape == (3, 64) and N * L * F < 2 ** 30
                    and _lib.load().emer_field_fwd_supported(L, F))


_RIDERS: dict = {}   # data_ptr of a neck's geometry features -> the rider whose rgb results were computed with them


def _versions(geo: Tensor, hray: Tensor, params) -> tuple:
    """Version counters of a colour query's tensors: an in-place write through torch between park and pick-up changes one of them (a write
    through ``.data`` or by a kernel on the raw pointer does not: after those, clear_riders())."""
    return (geo._version, hray._version) + tuple(p._version for p in params)


def clear_riders() -> None:
    for r in _RIDERS.values():
        r.geo = None
    _RIDERS.clear()
    ray_jobs.clear_fronts()


def _neck_fwd(enc: Tensor, W0, B0, W1, B1, n_out: int, want_h: bool):
    L, N, F = enc.shape
    h1 = _new(enc, N, 64) if want_h else None
    out0 = _new(enc, N, 64) if n_out > 1 else None
    out1 = _new(enc, N, 64) if n_out == 128 else None
    dens = _new(enc, N)
    _launch("emer_neck_fwd", enc, _p(enc), L, F, N, _p(W0), _p(B0), _p(W1), _p(B1), n_out, _p(h1), _p(out0), _p(out1), _p(dens))
    return h1, out0, out1, dens


def _neck_bwd(d0c, d1c, fa, dens, h, enc, W0, W1, n_out: int):
    """Data gradients of the neck (n_out 64 / 128) or the density MLP (n_out 1, fa = d dens) from the stored hidden layer -> (dpre1
    [N, 1] if n_out 1, col0, dpre0, denc).  col0 [N]: column 0 of the output layer's wgrad operand, d0[:, 0] + trunc_exp's gradient."""
    L, N, F = enc.shape
    dpre1 = _new(enc, N, 1) if n_out == 1 else None
    col0 = _new(enc, N) if (n_out > 1 and fa is not None) else None
    dpre0, denc = _new(enc, N, 64), _new(enc, L, N, F)
    _launch("emer_neck_bwd", enc, _p(d0c), _p(d1c), _p(fa), _p(dens), _p(h), L, F, N, _p(W0), _p(W1), n_out, _p(dpre1), _p(col0),
            _p(dpre0), _p(denc))
    return dpre1, col0, dpre0, denc


class _NeckFn(torch.autograd.Function):
    """(features 0..63, features 64..127 or None, density) = neck(enc_lm); density = trunc_exp(feature 0 - 1)."""

    @staticmethod
    def forward(ctx, enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, rider: Optional[RgbRider] = None):
        ctx.set_materialize_grads(False)
        enc, W0, B0, W1, B1 = _c(enc_lm), _c(w0), _c(b0), _c(w1), _c(b1)
        n_out = W1.shape[0]
        L, N, F = enc.shape
        need_grad = any(ctx.needs_input_grad)
        ctx.path = neck_path(L, F, N, n_out, need_grad)
        want_h = need_grad and ctx.path != "fused"
        if rider is not None and not want_h and rider.usable(L, F, N, n_out):
            h1, out1 = None, None
            out0, dens = _field_fwd(enc, W0, B0, W1, B1, rider)
        else:
            h1, out0, out1, dens = _neck_fwd(enc, W0, B0, W1, B1, n_out, want_h)
        ctx.save_for_backward(enc, W0, W1, h1, dens, B0)
        ctx.n_out = n_out
        ctx.sinks = tuple(_sink(p) for p in (w0, b0, w1, b1))
        return (out0, dens) if out1 is None else (out0, out1, dens)

    @staticmethod
    def backward(ctx, *grads):
        enc, W0, W1, h1, dens, B0 = ctx.saved_tensors
        n_out = ctx.n_out
        d0, d1, ddens = (grads[0], None, grads[1]) if n_out == 64 else grads
        if d0 is None and d1 is None and ddens is None:
            return None, None, None, None, None, None
        L, N, F = enc.shape
        d0c = None if d0 is None else _c(d0)
        d1c = None if d1 is None else _c(d1)
        fa = None if ddens is None else _c(ddens)
        # weight gradients accumulated straight into the parameters' .grad when the trainer allows it (_sink)
        (tw0, tb0, tw1, tb1), ret = _targets(ctx.sinks, _wb_shapes((W0, W1)), enc.device, last_layer_first=True)
        if ctx.path == "fused":
            # data gradients AND weight gradients in one kernel: neither h1 nor dpre0 reaches memory, enc / d are read once
            denc = _new(enc, L, N, F)
            ws = _new(enc, int(_lib.load().emer_neck_bwd_fused_workspace(L, F, N, n_out)))
            _launch("emer_neck_bwd_fused", enc, _p(d0c), _p(d1c), _p(fa), _p(dens), _p(enc), L, F, N, _p(W0), _p(B0), _p(W1), n_out,
                    _p(denc), _p(ws), _p(tw0), tw0.stride(0), _p(tb0), _p(tw1), tw1.stride(0), _p(tb1))
            return (denc, *ret, None)
        _, col0, dpre0, denc = _neck_bwd(d0c, d1c, fa, dens, h1, enc, W0, W1, n_out)
        # Output rows whose gradient is structurally zero (an unused semantic half) cost nothing.
        if d0c is None:
            d0c = torch.zeros((N, 64), device=enc.device, dtype=torch.float32)
        wgrad(d0c, [seg(h1, 0, 64)], 64, col0=col0, out_w=tw1[:64], out_b=tb1[:64])
        if n_out == 128 and d1c is not None:
            wgrad(d1c, [seg(h1, 0, 64)], 64, out_w=tw1[64:], out_b=tb1[64:])
        wgrad(dpre0, [seg_lm(enc, 0)], L * F, out_w=tw0, out_b=tb0)
        return (denc, *ret, None)


def _field_fwd(enc: Tensor, W0, B0, W1, B1, rider: RgbRider):
    """emer_field_fwd: the neck and the rider's rgb head in one launch; the rgb results are parked on the rider."""
    L, N, F = enc.shape
    hr = _c(rider.hray)
    RW0, RB0, RW1, RB1, RW2, RB2 = (_c(p) for p in rider.params)
    R, Kh = hr.shape
    geo, dens = _new(enc, N, 64), _new(enc, N)
    rb = ray_jobs.front_rb(rider.hray, rider.params[:4])   # already computed by the front launch on exactly these tensors?
    if rb is None:
        rb = _ray_pre_fwd(hr, RW0, RB0, RW1, RB1, enc)
    rec = rgb_recompute(R, rider.S) if rider.keep else 0   # [r6] recomputing backward: the activations it recomputes are not stored
    a1 = _new(enc, N, 64) if (rider.keep and rec != 1) else None
    a2 = _new(enc, N, 64) if (rider.keep and rec == 0) else None
    out = _new(enc, N, 3)
    _launch("emer_field_fwd", enc, _p(enc), L, F, R, rider.S, _p(W0), _p(B0), _p(W1), _p(B1), _p(rb), _p(rb[:, 64:]), 128, Kh,
            _p(RW0), _p(RW1), _p(RW2), _p(RB2), _p(geo), _p(dens), _p(a1), _p(a2), _p(out))
    rider.geo_ptr, rider.a1, rider.a2, rider.out, rider.rb = geo.data_ptr(), a1, a2, out, rb
    # what rgb_head needs to recognise these tensors, unchanged (the rule of ray_jobs.front_rb): their version counters now, and geo itself --
    # while the entry is parked its storage cannot be freed, so no other tensor can appear at its address
    rider.geo, rider.versions = geo, _versions(geo, rider.hray, rider.params)
    _RIDERS[geo.data_ptr()] = rider
    return geo, dens


def neck(enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor, rider: Optional[RgbRider] = None):
    """Register-resident neck: returns (feats[:, :64], feats[:, 64:128] or None, density [N]).  Requires
    ``neck_supported(L, F, hidden, n_out)`` with n_out in (64, 128).  ``rider``: a colour query on the resulting geometry
    features to evaluate in the same launch (see RgbRider)."""
    r = _NeckFn.apply(*_ng(enc_lm, w0, b0, w1, b1), rider)
    return (r[0], None, r[1]) if len(r) == 2 else r


# -------------------------------------------------------------------------------------- density MLP
class _DensityMLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor):
        ctx.set_materialize_grads(False)
        enc, W0, B0, W1, B1 = _c(enc_lm), _c(w0), _c(b0), _c(w1), _c(b1)
        L, N, F = enc.shape
        K0, H = L * F, W0.shape[0]
        need_grad = any(ctx.needs_input_grad)
        ctx.path = density_mlp_path(L, F, N, H, need_grad)
        ctx.sinks = tuple(_sink(p) for p in (w0, b0, w1, b1))
        if ctx.path != "chain":
            h, _, _, dens = _neck_fwd(enc, W0, B0, W1, B1, 1, need_grad and ctx.path != "fused")
            ctx.save_for_backward(enc, W0, W1, h, dens, B0)
            return dens
        h = _new(enc, N, H) if need_grad else None
        dens = _new(enc, N, 1)
        c_h = _r4(K0)
        # the output column lies past the K % 8 padding of layer 1: the kernel reads round_up(H, 8) columns from c_h (the tail
        # meets zero weights) and keeps the row buffer from tile to tile, so a density that overflowed to inf in a wave's
        # previous tile must not sit in that tail (inf * 0 = NaN on the same row of the wave's next tile)
        c_o = c_h + _ru(H, 8)
        run_chain([seg_lm(enc, 0)],
                  [layer(W0, B0, 0, c_h, ACT_RELU, store=h), layer(W1, B1, c_h, c_o, ACT_TRUNC_EXP, store=dens)],
                  c_o + 4, N, enc)
        ctx.save_for_backward(enc, W0, W1, h, dens, B0)
        return dens.view(N)

    @staticmethod
    def backward(ctx, ddens: Optional[Tensor]):
        enc, W0, W1, h, dens, B0 = ctx.saved_tensors
        if ddens is None:
            return None, None, None, None, None
        L, N, F = enc.shape
        K0, H = L * F, W0.shape[0]
        if ctx.path == "fused":
            denc = _new(enc, L, N, F)
            (tw0, tb0, tw1, tb1), ret = _targets(ctx.sinks, _wb_shapes((W0, W1)), enc.device)
            assert tw1.is_contiguous()
            ws = _new(enc, int(_lib.load().emer_density_bwd_fused_workspace(L, F, N)))
            _launch("emer_density_bwd_fused", enc, _p(_c(ddens).reshape(-1)), _p(dens), _p(enc), L, F, N, _p(W0), _p(B0), _p(W1), _p(denc), _p(ws),
                    _p(tw0), tw0.stride(0), _p(tb0), _p(tw1), _p(tb1))
            return (denc, *ret)
        if ctx.path == "neck_streamed":
            dpre1, _, dpre0, denc = _neck_bwd(None, None, _c(ddens), dens, h, enc, W0, W1, 1)
            (tw0, tb0, tw1, tb1), ret = _targets(ctx.sinks, _wb_shapes((W0, W1)), enc.device, last_layer_first=True)
            wgrad(dpre1, [seg(h, 0, H)], H, out_w=tw1, out_b=tb1)
            wgrad(dpre0, [seg_lm(enc, 0)], K0, out_w=tw0, out_b=tb0)
            return (denc, *ret)
        dpre1 = (_c(ddens).view(N, 1) * dens.view(N, 1).clamp(max=E15)).contiguous()
        dpre0, denc = _lm2_chain_bwd(seg(dpre1, 0, 1), 4, W0, W1, h, enc)
        dw1, db1 = wgrad(dpre1, [seg(h, 0, H)], H)
        dw0, db0 = wgrad(dpre0, [seg_lm(enc, 0)], K0)
        return denc, dw0, db0, dw1, db1


def density_mlp(enc_lm: Tensor, w0: Tensor, b0: Tensor, w1: Tensor, b1: Tensor) -> Tensor:
    """trunc_exp(Linear(ReLU(Linear(enc))) - 1) -> [N]."""
    L, N, F = enc_lm.shape
    if not neck_supported(L, F, w0.shape[0], 1) and not density_mlp_supported(L * F, w0.shape[0]):
        from . import ops   # too wide for one chain launch: layer by layer on emer_linear_*
        return ops.linear(ops.linear(ops.lm_to_rm(enc_lm), w0, b0, "relu"), w1, b1, "trunc_exp").view(N)
    return _DensityMLPFn.apply(*_ng(enc_lm, w0, b0, w1, b1))


# ------------------------------------------------------------------------------------------ rgb head
def _rgb_ray_tail(hr, W0, W1, s0, s1, tgt, ret, dgeo, g, deferred=None):
    """Per-ray tail of the register-resident rgb backward, from the per-ray sums s0 / s1 of dpre0 / dpre1 (8192-row GEMMs; colsum(s)
    is the bias gradient): hray's column blocks of dW0 / dW1 and both bias gradients (emer_ray_wgrad), d hray (emer_ray_pre_bwd), and
    the backward's return value.  deferred = (cap, ws): queued for the step's job launches, with the partials' reduction (cap)."""
    R, Kh = hr.shape
    H = W0.shape[0]
    tw0, tb0, tw1, tb1, tw2, tb2 = tgt
    wjobs = [(s1, [(hr, Kh, H)], tw1, tb1), (s0, [(hr, Kh, 0)], tw0, tb0)]
    if deferred is None:
        ray_wgrad(wjobs, g)
        dhray = _ray_pre_bwd(s0, s1, W0, W1, Kh, g)
    else:
        cap, ws = deferred
        dhray = _new(g, R, Kh)
        level_a = [ray_jobs.job(ray_jobs.PRE_BWD, ray_jobs.pre_bwd_args(s0, s1, Kh, W0, W1, dhray))]   # (the longer member first)
        if cap.n_jobs:
            level_a.append(ray_jobs.job(ray_jobs.DW_REDUCE, cap))
        ray_jobs.enqueue(level_a, [ray_jobs.wgrad_job(*j) for j in wjobs], (ws, s0, s1, hr, W0, W1, dhray, tw0, tb0, tw1, tb1, tw2, tb2), g,
                         outputs=[(dhray, hr)])
    return (dhray, dgeo, None, *ret, None, None)


class _RgbHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hray: Tensor, geo: Tensor, S: int, w0, b0, w1, b1, w2, b2, pre: Optional[RgbRider] = None, rb_front: Optional[Tensor] = None):
        ctx.set_materialize_grads(False)
        hr, W0, B0, W1, B1, W2, B2 = _c(hray), _c(w0), _c(b0), _c(w1), _c(b1), _c(w2), _c(b2)
        g = geo.detach()
        assert g.dtype == torch.float32 and g.dim() == 2 and g.stride(1) == 1
        N, NG = g.shape
        R, Kh = hr.shape
        assert R * S == N
        H, K0, C = W0.shape[0], Kh + NG, W2.shape[0]
        assert W0.shape[1] == K0 and W1.shape[1] == H + K0 and W2.shape[1] == H
        keep = any(ctx.needs_input_grad)  # inference (inputs detached by rgb_head): the fast kernel stores no activations
        ctx.path = path = rgb_head_path(R, S, Kh, H, NG, C, g.stride(0), g.data_ptr(), keep)
        ctx.S = S
        ctx.sinks = tuple(_sink(p) for p in (w0, b0, w1, b1, w2, b2))
        if path == "chain":   # [A1 | hray | geo]
            a1, a2, out = _skip_chain_fwd([(hr, Kh, dict(row_div=S)), (g, NG, dict(ld=g.stride(0)))], W0, B0, W1, B1, W2, B2, ACT_SIGMOID, N, g)
            ctx.save_for_backward(hr, g, W0, W1, W2, a1, a2, out, None)
            return out
        # [r6] the recomputing backward makes a1 / a2 from geo and the per-ray pre-activations: the forward then stores neither
        recompute = path in ("recompute_a1a2", "recompute_a2")
        store_a1, store_a2 = keep and path != "recompute_a1a2", keep and not recompute
        # (allocated before the rider is looked at, as always: a rider's step drops them unused, but the later allocations of a captured
        # step are carved from the blocks they hand back -- without them the replayed static step measured 1.2 % slower,
        # profiles/fused_paths_ab.json `allocation_order`)
        a1 = _new(g, N, H) if store_a1 else None
        a2 = _new(g, N, H) if store_a2 else None
        out = _new(g, N, C)
        if pre is not None and (pre.keep or not keep):
            # already evaluated inside the neck's launch on exactly these tensors (rgb_head checked): nothing to launch
            assert not keep or ((pre.a1 is None) == (not store_a1) and (pre.a2 is None) == (not store_a2)), \
                "rider and rgb head disagree about stored activations"
            ctx.save_for_backward(hr, g, W0, W1, W2, pre.a1, pre.a2, pre.out, pre.rb if recompute else None)
            return pre.out
        # per-ray part of layers 0 and 1 as per-ray pre-activations (ONE 8192-row launch instead of two 1M-row GEMMs)
        if rb_front is not None and rb_front.shape == (R, 2 * H):
            rb = rb_front   # the front launch evaluated it on exactly these tensors (rgb_head checked)
        else:
            rb = _ray_pre_fwd(hr, W0, B0, W1, B1, g)
        _launch("emer_rgb_head_fwd", g, _p(g), g.stride(0), _p(rb), _p(rb[:, H:]), rb.stride(0), R, S, Kh, _p(W0), _p(W1), _p(W2), _p(B2),
                _p(a1), _p(a2), _p(out))
        ctx.save_for_backward(hr, g, W0, W1, W2, a1, a2, out, rb if recompute else None)
        return out

    @staticmethod
    def backward(ctx, dout: Optional[Tensor]):
        hr, g, W0, W1, W2, a1, a2, out, rb = ctx.saved_tensors
        if dout is None:
            return (None,) * 11
        S, path = ctx.S, ctx.path
        N, NG = g.shape
        R, Kh = hr.shape
        H, K0, C = W0.shape[0], Kh + NG, W2.shape[0]
        assert H == _r4(H)
        dev = g.device
        if path == "chain":
            dpre2 = (_c(dout) * out * (1.0 - out)).contiguous()            # sigmoid'
            dh, dgeo = _new(g, N, Kh), _new(g, N, NG)
            dpre1, dpre0 = _skip_chain_bwd(dpre2, W0, W1, W2, a1, a2, [(0, Kh, dh), (Kh, K0, dgeo)], K0, g)
            dw2, db2 = wgrad(dpre2, [seg(a2, 0, H)], H)
            dw1, db1 = wgrad(dpre1, [seg(a1, 0, H), seg(hr, H, Kh, row_div=S), seg(g, H + Kh, NG, ld=g.stride(0))], H + K0)
            dw0, db0 = wgrad(dpre0, [seg(hr, 0, Kh, row_div=S), seg(g, Kh, NG, ld=g.stride(0))], K0)
            dhray = dh.view(R, S, Kh).sum(dim=1)
            return dhray, dgeo, None, dw0, db0, dw1, db1, dw2, db2, None, None
        dgeo, s1, s0 = _new(g, N, NG), _new(g, R, H), _new(g, R, H)
        tgt, ret = _targets(ctx.sinks, _wb_shapes((W0, W1, W2)), dev, last_layer_first=True)
        tw0, tb0, tw1, tb1, tw2, tb2 = tgt
        if path in _RGB_FUSED:
            # [r4] the weight gradients of the per-sample column blocks of layers 0 / 1 (and layer 2) inside the backward kernel:
            # dpre1 / dpre0 never reach memory and the two streamed weight-gradient launches are gone
            ws = _new(g, int(_lib.load().emer_rgb_head_bwd_fused_workspace(R, S)))
            # the per-ray tail (reduction of the partials, hray's weight-gradient blocks, d hray) may wait for the step's two job
            # launches (ray_jobs): only when hray is an output of _RayInputsFn of this forward (its backward flushes before it reads
            # d hray; torch consumers of other rows would not), and only into .grad itself -- a fresh tensor is added to .grad as
            # soon as this backward returns
            defer = ray_jobs.may_defer(hr) and all(t is not None for t in ctx.sinks)
            cap = ray_jobs.DwReduceArgs()
            rest = (R, S, Kh, _p(W0), _p(W1), _p(W2), _p(dgeo), _p(s1), _p(s0), _p(ws), _p(tw0), tw0.stride(0), _p(tw1), tw1.stride(0), _p(tw2),
                    tw2.stride(0), _p(tb2))
            with ray_jobs.capture_dw_reduce(cap) if defer else contextlib.nullcontext():
                if path == "fused":
                    _launch("emer_rgb_head_bwd_fused", g, _p(_c(dout)), _p(out), _p(a1), _p(a2), _p(g), g.stride(0), *rest)
                else:   # [r6] hidden activations recomputed from geo + the per-ray pre-activations (a1: stored unless recompute_a1a2)
                    _launch("emer_rgb_head_bwd_recompute", g, _p(_c(dout)), _p(out), _p(a1), _p(g), g.stride(0), _p(rb), _p(rb[:, H:]), rb.stride(0), *rest)
            return _rgb_ray_tail(hr, W0, W1, s0, s1, tgt, ret, dgeo, g, deferred=(cap, ws) if defer else None)
        # "w2_in_kernel": the output layer's weight gradient (3 x 64 + 3 numbers) rides along in the backward kernel, where a2 and
        # dpre2 are in registers (a separate pass would re-read 280 MB for it); "streamed": that one as a separate pass too
        w2_in = path == "w2_in_kernel"
        dpre2, dpre1, dpre0 = _new(g, N, C), _new(g, N, H), _new(g, N, H)
        ws = _new(g, int(_lib.load().emer_rgb_head_bwd_workspace(R))) if w2_in else None
        _launch("emer_rgb_head_bwd", g, _p(_c(dout)), _p(out), _p(a1), _p(a2), R, S, Kh, _p(W0), _p(W1), _p(W2), _p(dpre2), _p(dpre1),
                _p(dpre0), _p(dgeo), _p(s1), _p(s0), _p(ws), _p(tw2) if w2_in else None, tw2.stride(0), _p(tb2) if w2_in else None)
        if not w2_in:
            wgrad(dpre2, [seg(a2, 0, H)], H, out_w=tw2, out_b=tb2)
        # per-sample column blocks [A1 | . | geo] of dW1 and [. | geo] of dW0
        wgrad(dpre1, [seg(a1, 0, H, dst_col=0), seg(g, H, NG, ld=g.stride(0), dst_col=H + Kh)], H + NG, want_bias=False, out_w=tw1)
        wgrad(dpre0, [seg(g, 0, NG, ld=g.stride(0), dst_col=Kh)], NG, want_bias=False, out_w=tw0)
        return _rgb_ray_tail(hr, W0, W1, s0, s1, tgt, ret, dgeo, g)


def rgb_head(hray: Tensor, geo: Tensor, samples_per_ray: int, w0, b0, w1, b1, w2, b2) -> Tensor:
    """sigmoid(MLP3-skip1([hray[ray] | geo])) -> [N, 3]; hray [R, Kh] per ray, geo [N, NG] per sample."""
    if not rgb_head_supported(w0.shape[0], hray.shape[1], geo.shape[1], w2.shape[0]):
        # too wide for one chain launch: the concatenated rows, layer by layer on emer_linear_*
        return _skip3_layers(torch.cat([hray.repeat_interleave(samples_per_ray, dim=0), geo], dim=-1), w0, b0, w1, b1, w2, b2, ACT_SIGMOID)
    pre = _RIDERS.pop(geo.data_ptr(), None)
    if pre is not None:  # the same query, tensor for tensor and unchanged since, that rode along in the neck's launch?
        same = (pre.S == samples_per_ray and pre.hray.data_ptr() == hray.data_ptr() and pre.hray.shape == hray.shape
                and geo.dim() == 2 and geo.shape[1] == 64 and geo.stride(0) == 64
                and all(a is b for a, b in zip(pre.params, (w0, b0, w1, b1, w2, b2)))
                and pre.versions == _versions(geo, hray, pre.params))
        pre.geo = None   # no longer parked: the features live as long as their users hold them
        pre = pre if same else None
    rb_front = ray_jobs.front_rb(hray, (w0, b0, w1, b1)) if pre is None else None
    return _RgbHeadFn.apply(*_ng(hray, geo, samples_per_ray, w0, b0, w1, b1, w2, b2), pre, rb_front)


# ------------------------------------------------------------------------------------------ per-ray inputs
class _RayInputsFn(torch.autograd.Function):
    """Input rows of the rgb head ([PE((d+1)/2) | emb[idx]]) and of the sky head ([PE(d) | emb[idx]]) in ONE launch
    (radiance_field.py:622-643,660-674; replaces two encoder launches, the gather and two cats), and the embedding
    table's gradient as one deterministic segment sum over both consumers' input gradients (replaces autograd's add,
    a zero fill and an atomic index_add)."""

    @staticmethod
    def forward(ctx, weight: Tensor, idx: Tensor, dirs: Tensor, max_deg: int, front=None):
        ctx.set_materialize_grads(False)
        w = _c(weight)
        assert idx.dtype == torch.int64 and idx.dim() == 1 and dirs.dim() == 2 and dirs.dtype == torch.float32 and dirs.stride(1) == 1
        R, E = dirs.shape[0], w.shape[1]
        P = 3 if max_deg == 0 else 3 * (1 + 2 * (max_deg + 1))
        dev = dirs.device
        with torch.cuda.device(dev):
            out_rgb, out_sky = _new(dev, R, P + E), _new(dev, R, P + E)
            if not (ray_jobs.ENABLED and front is not None and _front_launch(front, w, idx, dirs, max_deg, out_rgb, out_sky)):
                _lib.call("emer_ray_inputs_fwd", _p(dirs), dirs.stride(0), _p(idx), idx.stride(0), _p(w), w.shape[0], E, max_deg, R,
                          _p(out_rgb), P + E, _p(out_sky), P + E, _stream(dirs))
        ctx.save_for_backward(idx)
        ctx.sink, ctx.shape, ctx.P = _sink(weight), tuple(w.shape), P
        ctx.out_ptrs = (out_rgb.data_ptr(), out_sky.data_ptr())
        ray_jobs.register_rows(out_rgb, out_sky)   # the only inputs whose gradient a head may defer: it comes back to THIS node
        return out_rgb, out_sky

    @staticmethod
    def backward(ctx, g_rgb: Optional[Tensor], g_sky: Optional[Tensor]):
        if g_rgb is None and g_sky is None:
            return None, None, None, None, None
        (idx,) = ctx.saved_tensors
        dev = idx.device
        P = ctx.P
        # a head's backward that deferred its per-ray jobs handed back the tensor those jobs will WRITE: legal only if that very
        # tensor arrives here (one consumer per input; a second one would have made autograd add unwritten memory on the way)
        ray_jobs.check_single_consumer(ctx.out_ptrs[0], g_rgb)
        ray_jobs.check_single_consumer(ctx.out_ptrs[1], g_sky)

        def cols(g):
            if g is None:
                return None, 0
            if not (g.dtype == torch.float32 and g.stride(1) == 1):
                ray_jobs.flush()   # (a converted copy must see the written gradient)
                g = g.to(torch.float32).contiguous()
            return g[:, P:], g.stride(0)

        (ga, lda), (gb, ldb) = cols(g_rgb), cols(g_sky)
        tw, rw = _target(ctx.sink, ctx.shape, dev)
        if ray_jobs.armed():
            # launch A (what the heads queued: their row-local chains, the reduction) and launch B (their weight gradients and this
            # table's gradient, which reads the input gradients launch A writes)
            ray_jobs.flush([ray_jobs.job(ray_jobs.EMBED_GRAD, ray_jobs.embed_grad_args(ga, lda, gb, ldb, idx, ctx.shape[0], ctx.shape[1], tw))], idx)
            return rw, None, None, None, None
        _launch("emer_embed_grad", idx, _p(ga), lda, _p(gb), ldb, _p(idx), idx.stride(0), idx.shape[0], ctx.shape[0], ctx.shape[1],
                _p(tw))
        return rw, None, None, None, None


def _plain(p) -> bool:
    return isinstance(p, Tensor) and p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()


def _front_launch(front, w: Tensor, idx: Tensor, dirs: Tensor, max_deg: int, out_rgb: Tensor, out_sky: Tensor) -> bool:
    """The FRONT launch (ray_jobs): both heads' input rows and, in the same launch and the same workgroups, what each head computes
    from its rows alone -- the rgb head's per-ray pre-activations, the whole sky head.  front = (rgb head's (w0 .. b2) | None,
    sky head's (w0 .. b2) | None, the sky head's final activation).  The results are parked for _field_fwd / rgb_head / skip_mlp3,
    which take them only for the very same input and parameters; False: nothing to fuse (the caller launches the plain kernel)."""
    rgb_p, sky_p, sky_act = front
    R, K = out_rgb.shape
    fits = lambda p: p is not None and len(p) == 6 and all(_plain(t) for t in p) and K <= 64 and p[0].shape[0] == 64 and p[2].shape[0] == 64
    rgb_ok = fits(rgb_p) and rgb_p[0].shape[1] >= K and rgb_p[2].shape[1] >= 64 + K
    sky_ok = (fits(sky_p) and sky_p[0].shape == (64, K) and sky_p[2].shape == (64, 64 + K) and sky_p[4].shape[1] == 64
              and sky_p[4].shape[0] <= 16 and sky_act in (ACT_NONE, ACT_SIGMOID))
    if not (rgb_ok or sky_ok) or R == 0:
        return False
    dev = out_rgb.device
    parked = ray_jobs.Front()
    jobs = []
    if sky_ok:   # the longer chain first
        W0, B0, W1, B1, W2, B2 = (p.detach() for p in sky_p)
        C = W2.shape[0]
        rb, a1, a2, out = _new(dev, R, 128), _new(dev, R, 64), _new(dev, R, 64), _new(dev, R, C)
        jobs.append(ray_jobs.fwd_chain_job(ray_jobs.inputs_args(dirs, idx, w, max_deg, None, out_sky), ray_jobs.pre_fwd_args(out_sky, W0, B0, W1, B1, rb),
                                           ray_jobs.head_fwd_args(rb, W1, W2, B2, sky_act, a1, a2, out)))
        parked.sky = (out_sky, tuple(sky_p), tuple(p._version for p in sky_p), sky_act, (rb, a1, a2, out))
    else:
        jobs.append(ray_jobs.job(ray_jobs.INPUTS, ray_jobs.inputs_args(dirs, idx, w, max_deg, None, out_sky)))
    if rgb_ok:
        W0, B0, W1, B1 = (p.detach() for p in rgb_p[:4])
        rb = _new(dev, R, 128)
        jobs.append(ray_jobs.fwd_chain_job(ray_jobs.inputs_args(dirs, idx, w, max_deg, out_rgb, None), ray_jobs.pre_fwd_args(out_rgb, W0, B0, W1, B1, rb)))
        parked.rgb = (out_rgb, tuple(rgb_p[:4]), tuple(p._version for p in rgb_p[:4]), rb)
    else:
        jobs.append(ray_jobs.job(ray_jobs.INPUTS, ray_jobs.inputs_args(dirs, idx, w, max_deg, out_rgb, None)))
    ray_jobs.launch(jobs, dirs)
    ray_jobs.park(out_rgb, out_sky, parked)
    return True


def ray_inputs(emb_weight: Tensor, idx: Tensor, dirs: Tensor, max_deg: int, front=None):
    """(rgb-head rows, sky-head rows), each [R, PE + emb_dim], for per-ray directions [R, 3] and embedding indices [R].
    ``front``: the heads that will consume the rows (see _front_launch), to evaluate their per-ray stages in the same launch."""
    return _RayInputsFn.apply(*_ng(emb_weight, idx, dirs, max_deg), front)


# ------------------------------------------------------------------------- 3-layer skip MLP on row-major input
class _SkipMLP3Fn(torch.autograd.Function):
    """act(MLP(x)) for mlp.MLP(num_layers=3, skip_connections=[1]) (mlp.py:20-46) on a plain row-major input -- the
    per-ray sky head (radiance_field.py:156-187,660-686).  Two small launches each way (or one chain launch), instead of
    three Linear launches each way with [rows, 64] round trips."""

    @staticmethod
    def forward(ctx, x: Tensor, w0, b0, w1, b1, w2, b2, final_act: int, front=None):
        ctx.set_materialize_grads(False)
        X, W0, B0, W1, B1, W2, B2 = _c(x), _c(w0), _c(b0), _c(w1), _c(b1), _c(w2), _c(b2)
        N, K0 = X.shape
        H, C = W0.shape[0], W2.shape[0]
        assert W0.shape[1] == K0 and W1.shape[1] == H + K0 and W2.shape[1] == H and H % 4 == 0
        ctx.path = skip_mlp3_path(N, K0, H, C, any(ctx.needs_input_grad))
        ctx.final_act = final_act
        ctx.sinks = tuple(_sink(p) for p in (w0, b0, w1, b1, w2, b2))
        if front is not None and ctx.path != "chain" and X.data_ptr() == x.data_ptr():
            # already evaluated by the front launch on exactly these tensors (skip_mlp3 checked): nothing to launch
            _, a1, a2, out = front
            assert a1.shape == (N, H) and a2.shape == (N, H) and out.shape == (N, C)
            ctx.save_for_backward(X, W0, W1, W2, a1, a2, out)
            return out.view_as(out)   # (a fresh tensor object for autograd; the parked one stays as it is)
        if ctx.path == "chain":   # [A1 | x]
            a1, a2, out = _skip_chain_fwd([(X, K0, {})], W0, B0, W1, B1, W2, B2, final_act, N, X)
        else:
            # the input's share of layers 0 and 1, then the rest of the MLP
            a1, a2, out = _new(X, N, H), _new(X, N, H), _new(X, N, C)
            rb = _ray_pre_fwd(X, W0, B0, W1, B1, X)
            _launch("emer_ray_head_fwd", X, _p(rb), 2 * H, N, _p(W1), W1.stride(0), _p(W2), _p(B2), C, final_act, _p(a1), _p(a2), _p(out))
        ctx.save_for_backward(X, W0, W1, W2, a1, a2, out)
        return out

    @staticmethod
    def backward(ctx, dout: Optional[Tensor]):
        X, W0, W1, W2, a1, a2, out = ctx.saved_tensors
        if dout is None:
            return (None,) * 9
        N, K0 = X.shape
        H, C = W0.shape[0], W2.shape[0]
        path = ctx.path
        d = _c(dout)
        tgt, ret = _targets(ctx.sinks, _wb_shapes((W0, W1, W2)), X.device, last_layer_first=True)
        tw0, tb0, tw1, tb1, tw2, tb2 = tgt
        if path == "chain":
            dpre2 = torch.ops.aten.sigmoid_backward(d, out) if ctx.final_act == ACT_SIGMOID else d  # sigmoid' (one launch) / identity
            dx = _new(X, N, K0)
            dpre1, dpre0 = _skip_chain_bwd(dpre2, W0, W1, W2, a1, a2, [(0, K0, dx)], _r4(K0), X)
        else:
            dpre2, dpre1, dpre0 = _new(X, N, C), _new(X, N, H), _new(X, N, H)
            wjobs = [(dpre2, [(a2, H, 0)], tw2, tb2), (dpre1, [(a1, H, 0), (X, K0, H)], tw1, tb1), (dpre0, [(X, K0, 0)], tw0, tb0)]
            if path == "ray" and ray_jobs.may_defer(X) and all(t is not None for t in ctx.sinks):
                # the whole backward waits for the step's two job launches (ray_jobs): the row-local chain in the first, the weight
                # gradients in the second (only into .grad itself: a fresh tensor is added to .grad as soon as this backward returns)
                dx = _new(X, N, K0)
                chain = ray_jobs.bwd_chain_job(ray_jobs.head_bwd_args(d, out, a1, a2, W1, W2, ctx.final_act, dpre2, dpre1, dpre0),
                                               ray_jobs.pre_bwd_args(dpre0, dpre1, K0, W0, W1, dx))
                ray_jobs.enqueue([chain], [ray_jobs.wgrad_job(*j) for j in wjobs],
                                 (d, out, a1, a2, X, W0, W1, W2, dpre2, dpre1, dpre0, dx, tw0, tb0, tw1, tb1, tw2, tb2), X, outputs=[(dx, X)])
                return (dx, *ret, None, None)
            _launch("emer_ray_head_bwd", X, _p(d), _p(out), _p(a1), _p(a2), N, _p(W1), W1.stride(0), _p(W2), C, ctx.final_act, _p(dpre2),
                    _p(dpre1), _p(dpre0))
            dx = _ray_pre_bwd(dpre0, dpre1, W0, W1, K0, X)
        if path == "ray":   # per-ray head: all three layers' weight gradients in one launch
            ray_wgrad(wjobs, X)
        else:
            wgrad(dpre2, [seg(a2, 0, H)], H, out_w=tw2, out_b=tb2)
            wgrad(dpre1, [seg(a1, 0, H), seg(X, H, K0)], H + K0, out_w=tw1, out_b=tb1)
            wgrad(dpre0, [seg(X, 0, K0)], K0, out_w=tw0, out_b=tb0)
        return (dx, *ret, None, None)


def skip_mlp3(x: Tensor, w0, b0, w1, b1, w2, b2, final_act: int = ACT_SIGMOID) -> Tensor:
    """final_act(MLP3-skip1(x)) for x [rows, K0]; final_act ACT_SIGMOID or ACT_NONE."""
    assert final_act in (ACT_SIGMOID, ACT_NONE)
    if not skip_mlp3_supported(w0.shape[0], x.shape[1], w2.shape[0]):
        return _skip3_layers(x, w0, b0, w1, b1, w2, b2, final_act)   # too wide for one chain launch
    front = ray_jobs.front_sky(x, (w0, b0, w1, b1, w2, b2), final_act)
    return _SkipMLP3Fn.apply(*_ng(x, w0, b0, w1, b1, w2, b2, final_act), front)


# ----------------------------------------------------------------- plain nn.Sequential heads (shadow / flow / dino)
def seq_mlp_supported(weights) -> bool:
    """2..4 Linear layers whose weights fit the chain kernel's LDS budget and column buffer."""
    if not (2 <= len(weights) <= 4):
        return False
    lds = sum((-(-w.shape[0] // 16) * 16) * ((-(-w.shape[1] // 8) * 8) + 2) * 4 for w in weights)
    cols = _r4(weights[0].shape[1]) + sum(_r4(w.shape[0]) for w in weights)
    if not (lds <= 96 * 1024 and cols <= 500 and all(w.shape[0] <= 256 for w in weights)):
        return False
    return _all_fit(seq_mlp_chain_shapes([w.shape[1] for w in weights] + [weights[-1].shape[0]]))


def seq_mlp_chain_shapes(dims):
    """[(buf_cols, [(K, N) per layer])] of seq_mlp's forward and backward (with dx) chains for Linear widths dims[0] -> ... -> dims[-1]."""
    n = len(dims) - 1
    fwd = (_r4(dims[0]) + sum(_r4(d) for d in dims[1:]), [(dims[i], dims[i + 1]) for i in range(n)])
    bwd = (sum(_r4(d) for d in dims), [(dims[i + 1], dims[i]) for i in range(n - 1, -1, -1)])
    return [fwd, bwd]


class _SeqMLPFn(torch.autograd.Function):
    """final_act(Linear_n(ReLU(... ReLU(Linear_1(x))))) -- the shadow head (radiance_field.py:148-153), flow MLP
    (:101-111) and dino heads (:192-198) as ONE chain launch forward and one for the data gradients."""

    @staticmethod
    def forward(ctx, x: Tensor, final_act: int, *wb):
        ctx.set_materialize_grads(False)
        X = _c(x)
        Ws, Bs = _split_wb(wb)
        N, K0 = X.shape
        n = len(Ws)
        ctx.path = "chain"
        cols = [0, _r4(K0)]
        for w in Ws:
            cols.append(cols[-1] + _r4(w.shape[0]))
        acts = [_new(X, N, w.shape[0]) for w in Ws]
        layers = [layer(Ws[i], Bs[i], cols[i], cols[i + 1], ACT_RELU if i + 1 < n else final_act, store=acts[i]) for i in range(n)]
        run_chain([seg(X, 0, K0)], layers, cols[-1], N, X)
        ctx.save_for_backward(X, *Ws, *acts)
        ctx.n, ctx.final_act = n, final_act
        ctx.sinks = tuple(_sink(p) for p in wb)
        ctx.need_dx = ctx.needs_input_grad[0]
        return acts[-1]

    @staticmethod
    def backward(ctx, dout: Optional[Tensor]):
        n = ctx.n
        if dout is None:
            return (None,) * (2 + 2 * n)
        saved = ctx.saved_tensors
        X, Ws, acts = saved[0], saved[1:1 + n], saved[1 + n:]
        N, K0 = X.shape
        d = _c(dout)
        out = acts[-1]
        dlast = (d * out * (1.0 - out)).contiguous() if ctx.final_act == ACT_SIGMOID else d
        dpre = [None] * n
        dpre[n - 1] = dlast
        cols = [0, _r4(Ws[n - 1].shape[0])]
        layers = []
        for i in range(n - 1, 0, -1):      # dA_{i-1} = dPre_i W_i, masked by relu'(act_{i-1}) -> dPre_{i-1}
            dpre[i - 1] = _new(X, N, Ws[i].shape[1])
            cols.append(cols[-1] + _r4(Ws[i].shape[1]))
            layers.append(layer(Ws[i], None, cols[-3], cols[-2], transposed=True, mask=acts[i - 1], store=dpre[i - 1]))
        dx = None
        if ctx.need_dx:
            dx = _new(X, N, K0)
            cols.append(cols[-1] + _r4(K0))
            layers.append(layer(Ws[0], None, cols[-3], cols[-2], transposed=True, store=dx))
        if layers:
            run_chain([seg(dlast, 0, Ws[n - 1].shape[0])], layers, cols[-1], N, X)
        operands = [[seg(X if i == 0 else acts[i - 1], 0, Ws[i].shape[1])] for i in range(n)]
        need_b = [ctx.needs_input_grad[2 + 2 * i + 1] for i in range(n)]
        return (dx, None, *_stack_wgrads(dpre, operands, Ws, ctx.sinks, need_b, X.device))


# ------------------------------------------------------------- plain 2- / 3-layer heads (register-resident)
def rmlp_supported(weights, k0: int, n_feat: int) -> bool:
    """Linear(k0, 64)-ReLU-[Linear(64, 64)-ReLU-]Linear(64, n_out <= 64) on row-major (n_feat 0) or level-major input."""
    n = len(weights)
    if n not in (2, 3):
        return False
    if any(w.shape[0] != 64 for w in weights[:-1]) or any(w.shape[1] != 64 for w in weights[1:]) or weights[0].shape[1] != k0:
        return False
    return bool(_lib.load().emer_rmlp_supported(n, k0, n_feat, 64, weights[-1].shape[0]))


class _RMlpFn(torch.autograd.Function):
    """final_act(Linear(ReLU(... ReLU(Linear(x))))) with hidden width 64 as ONE register-resident kernel each way
    (csrc/mlp_fused.hip: rmlp_fwd / rmlp_bwd): the flow MLP on the level-major xyzt encoding (radiance_field.py:101-111,
    359-389), the shadow head (:148-153) and the feature heads (:192-198)."""

    @staticmethod
    def forward(ctx, x: Tensor, level_major: bool, final_act: int, *wb):
        ctx.set_materialize_grads(False)
        X = _c(x)
        Ws, Bs = _split_wb(wb)
        n = len(Ws)
        L, F, N, K0 = _stack_shape(X, level_major)
        n_out = Ws[-1].shape[0]
        need_bwd = any(ctx.needs_input_grad)
        ctx.path = seq_mlp_path(Ws, F, N, need_bwd, all(b is not None for b in Bs[:n - 1]))
        keep = need_bwd and ctx.path != "fused"
        h1 = _new(X, N, 64) if keep else None
        h2 = _new(X, N, 64) if (keep and n == 3) else None
        out = _new(X, N, n_out)
        w2, b2 = (Ws[2], Bs[2]) if n == 3 else (None, None)
        _launch("emer_rmlp_fwd", X, _p(X), (0 if level_major else K0), L, F, K0, N, n, _p(Ws[0]), _p(Bs[0]), _p(Ws[1]), _p(Bs[1]), _p(w2), _p(b2),
                n_out, final_act, _p(h1), _p(h2), _p(out), n_out)
        if ctx.path == "fused":
            ctx.save_for_backward(X, out, *Ws, *Bs[:n - 1])
        else:
            ctx.save_for_backward(X, out, *Ws, *([h1] if h1 is not None else []), *([h2] if h2 is not None else []))
        ctx.n, ctx.final_act, ctx.level_major = n, final_act, level_major
        ctx.sinks = tuple(_sink(p) for p in wb)
        ctx.need_dx = ctx.needs_input_grad[0]
        return out

    @staticmethod
    def backward(ctx, dout: Optional[Tensor]):
        n = ctx.n
        if dout is None:
            return (None,) * (3 + 2 * n)
        saved = ctx.saved_tensors
        X, out, Ws = saved[0], saved[1], saved[2:2 + n]
        L, F, N, K0 = _stack_shape(X, ctx.level_major)
        ldx = 0 if ctx.level_major else K0
        n_out = Ws[-1].shape[0]
        d = _c(dout)
        need_b = [ctx.needs_input_grad[3 + 2 * i + 1] for i in range(n)]
        w2 = Ws[2] if n == 3 else None
        if ctx.path == "fused":
            Bh = saved[2 + n:2 + n + n - 1]   # biases of the hidden layers (the recomputation needs them)
            dx = torch.empty_like(X) if ctx.need_dx else None
            tgt, ret = _targets(ctx.sinks, _wb_shapes(Ws, need_b), X.device)
            ws = _new(X, int(_lib.load().emer_rmlp_bwd_fused_workspace(n, K0, F, N, n_out)))
            b1 = Bh[1] if n == 3 else None
            tw2, tb2 = (tgt[4], tgt[5]) if n == 3 else (None, None)
            _launch("emer_rmlp_bwd_fused", X, _p(d), d.stride(0), _p(out), out.stride(0), _p(X), (0 if ctx.level_major else X.stride(0)), L, F, K0, N, n,
                    _p(Ws[0]), _p(Bh[0]), _p(Ws[1]), _p(b1), _p(w2), n_out, ctx.final_act, _p(dx), ldx, _p(ws),
                    _p(tgt[0]), tgt[0].stride(0), _p(tgt[1]), _p(tgt[2]), tgt[2].stride(0), _p(tgt[3]),
                    _p(tw2), (tw2.stride(0) if tw2 is not None else 0), _p(tb2))
            return (dx, None, None, *ret)
        h1 = saved[2 + n]
        h2 = saved[3 + n] if n == 3 else None
        dlast = (d * out * (1.0 - out)).contiguous() if ctx.final_act == ACT_SIGMOID else d
        dpre0 = _new(X, N, 64)
        dpre1 = _new(X, N, 64) if n == 3 else None
        dx = torch.empty_like(X) if ctx.need_dx else None
        _launch("emer_rmlp_bwd", X, _p(dlast), n_out, _p(h1), _p(h2), L, F, K0, N, n, _p(Ws[0]), _p(Ws[1]), _p(w2), n_out,
                _p(dpre1), _p(dpre0), _p(dx), ldx)
        dpre = [dpre0, dpre1, dlast] if n == 3 else [dpre0, dlast]
        operands = [[seg_lm(X, 0)] if ctx.level_major else [seg(X, 0, K0)], [seg(h1, 0, 64)]] + ([[seg(h2, 0, 64)]] if n == 3 else [])
        return (dx, None, None, *_stack_wgrads(dpre, operands, Ws, ctx.sinks, need_b, X.device))


def seq_mlp(x: Tensor, weights, biases, final_act: int = ACT_NONE) -> Tensor:
    """Fused nn.Sequential(Linear, ReLU, ..., Linear[, Sigmoid]); x [rows, K0] row-major.  Stacks of hidden width 64
    run on the register-resident kernels, everything else on the LDS-staged chain."""
    assert final_act in (ACT_NONE, ACT_SIGMOID)
    wb = [t for pair in zip(weights, biases) for t in pair]
    if x.shape[-1] % 4 == 0 and rmlp_supported(weights, x.shape[-1], 0):
        return _RMlpFn.apply(*_ng(x, False, final_act, *wb))
    if not seq_mlp_supported(weights):
        from . import ops   # too wide (or too deep) for one chain launch: layer by layer on emer_linear_*
        n = len(weights)
        for i, (w, b) in enumerate(zip(weights, biases)):
            x = ops.linear(x, w, b, "relu" if i + 1 < n else ("sigmoid" if final_act == ACT_SIGMOID else None))
        return x
    return _SeqMLPFn.apply(*_ng(x, final_act, *wb))


def seq_mlp_lm(enc_lm: Tensor, weights, biases, final_act: int = ACT_NONE) -> Tensor:
    """The same stack fed by a LEVEL-MAJOR grid encoding [L, N, F] (no row-major copy of the encoding, the input gradient
    comes back level-major for the grid backward).  Requires ``rmlp_supported(weights, L * F, F)``."""
    assert final_act in (ACT_NONE, ACT_SIGMOID)
    wb = [t for pair in zip(weights, biases) for t in pair]
    return _RMlpFn.apply(*_ng(enc_lm, True, final_act, *wb))
