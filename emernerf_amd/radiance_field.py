"""RadianceField / DensityField with the reference's interface on the HIP kernels.

Mirrors radiance_fields/radiance_field.py (and radiance_fields/mlp.py) of the reference: same
constructor arguments, same sub-module / parameter names (reference checkpoints load with
``load_state_dict``), same ``forward`` contract, same default initialisation order
(so ``torch.manual_seed`` reproduces the reference's nn.Linear weights).  The arithmetic runs in
``emernerf_amd.ops`` (hand-written HIP): hash-grid encode/backward, contraction, fp32-MFMA linear layers
with fused ReLU / sigmoid / density epilogues.  torch itself only supplies parameter containers,
``torch.cat`` / indexing glue, the appearance-embedding gather and ``grid_sample`` for the (optional)
learnable PE map.

Which entry points a forward runs is decided ONCE, on entry, by ``RadianceField._routes`` from the pure rules below (``neck_eligible``,
``flow_mlp_eligible``, ``skip_head_params``, ``appearance_key``) and kept as ``last_routes``, a dict of strings for tests and tools (the
analogue of ``ctx.path`` in fused.py).  The helpers are handed their route; a public method called directly computes its own through the
same rules.  "none": the stage does not run.  Route, value, condition -> entry points:
  static     neck          neck_eligible(static grid, base_mlp) -> fused.neck;  chain: otherwise -> fused.base_mlp, torch.split
  dynamic    neck          neck_eligible(dynamic grid, dynamic_base_mlp) -> fused.neck (+ ops.lm_to_rm for the hash encodings)
             chain         otherwise, no flow field -> fused.base_mlp, torch.split
             sequential    otherwise, flow field (it wants the row-major hash encodings) -> row-major encode, _run_sequential
  flow       interpolated  enable_temporal_interpolation in eval mode -> call_by_call through _flow_hash_interpolated, where the timestamps
                           of each evaluation (data, no route: one host read) choose between interpolation and the plain evaluation
             batched       BATCH_XYZT, positions given, dynamic neck, flow_mlp fused -> _flow_branch: 3 encodes, fused.neck,
                           2 fused.seq_mlp_lm, ops.aggregate3_density / aggregate3
             call_by_call  otherwise -> forward_dynamic_hash, forward_flow_hash, temporal_aggregation: 6 encodes
  flow_mlp   fused         flow_mlp_eligible(flow_mlp, flow grid) -> fused.seq_mlp_lm;  sequential: otherwise -> row-major encode, _run_sequential
  warp       fused         batched, FUSE_FLOW_WARP, 3-D, no gradient into positions or xyzt -> ops.flow_warp;  torch: batched otherwise -> _warp
  rgb        rider         per_ray and FUSE_FIELD, static neck on (R, S, 3) points, ray_inputs shared, 64-wide head -> fused.RgbRider offered
                           to the neck's launch (taken where RgbRider.usable); fused.rgb_head picks its results up
             per_ray       stride-0 (R, S, 3) directions, appearance index per ray or absent, skip head of width % 4 -> fused.rgb_head
             general       otherwise -> direction encoding, torch.cat, MLP on ops.linear
  sky        ray_chain     skip head of width % 4 -> fused.skip_mlp3;  module: otherwise -> MLP on ops.linear
  ray_inputs shared        _ray_rows_args: an indexed embedding, int64 per-ray indices, fp32 per-ray directions without gradient
                           -> ONE fused.ray_inputs launch makes the rows of the rgb and of the sky head
             separate      otherwise -> direction encoding and _EmbedFn per head, the per-ray gather still shared (the sky head of
                           (R, S, 3) directions that are no broadcast: a fused.ray_inputs launch of its own)
"""
from __future__ import annotations

import os

import logging
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _lib, fused, ops
from .encodings import HashEncoder, SinusoidalEncoder, build_xyz_encoder_from_cfg

logger = logging.getLogger()


def _run_sequential(seq: nn.Sequential, x: Tensor) -> Tensor:
    """Evaluate nn.Sequential(Linear, ReLU, ..., Linear[, Sigmoid]) with fused-activation HIP linears."""
    mods = list(seq)
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    # plain Linear-ReLU-...-Linear[-Sigmoid] stacks on row-major input: one fused chain launch each way
    body = mods[:-1] if isinstance(mods[-1], nn.Sigmoid) else mods
    pattern_ok = len(body) % 2 == 1 and all(isinstance(m, nn.Linear if j % 2 == 0 else nn.ReLU) for j, m in enumerate(body))
    if pattern_ok and x.is_cuda and all(l.bias is not None for l in lins) and fused.seq_mlp_supported([l.weight for l in lins]):
        lead = x.shape[:-1]
        y = fused.seq_mlp(x.reshape(-1, x.shape[-1]), [l.weight for l in lins], [l.bias for l in lins],
                          _lib.ACT_SIGMOID if isinstance(mods[-1], nn.Sigmoid) else _lib.ACT_NONE)
        return y.view(*lead, -1)
    for i, m in enumerate(mods):   # layer by layer, each Linear with the activation that follows it
        if isinstance(m, nn.Linear):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            x = ops.linear(x, m.weight, m.bias, "relu" if isinstance(nxt, nn.ReLU) else "sigmoid" if isinstance(nxt, nn.Sigmoid) else None)
        else:
            assert i > 0 and isinstance(m, (nn.ReLU, nn.Sigmoid)) and isinstance(mods[i - 1], nn.Linear), f"unexpected module {type(m)} in head"
    return x


# ------------------------------------------------------------------ the rules (pure: shapes, flags, fused.*_supported, plain values)
def neck_eligible(geometry_dim: int, semantic_dim: int, n_levels: int, n_feat: int, hidden: int, n_out: int) -> bool:
    """fused.neck covers this grid + Linear-ReLU-Linear: 64 geometry features, output [geometry | semantic], a shape the kernel has."""
    return bool(geometry_dim == 64 and n_out == 64 + semantic_dim and fused.neck_supported(n_levels, n_feat, hidden, n_out))


def flow_mlp_eligible(weights, biases, n_levels: int, n_feat: int) -> bool:
    """fused.seq_mlp_lm covers the flow MLP on the level-major xyzt encoding: three Linears, all biased, widths the kernel has."""
    return bool(len(weights) == 3 and all(b is not None for b in biases) and fused.rmlp_supported(weights, n_levels * n_feat, n_feat))


WIDTH_64 = "64"        # the per-ray kernels and the rider: hidden width exactly 64
WIDTH_CHAIN = "% 4"    # the chain (fused.rgb_head / fused.skip_mlp3 sort out what fits one launch): any multiple of 4


def skip_head_params(head, width: str) -> Optional[tuple]:
    """(w0, b0, w1, b1, w2, b2) of a 3-layer, skip-at-1, biased head (the rgb / sky MLP) whose hidden width meets ``width``, else None."""
    if (head is None or len(head.layers) != 3 or list(head.skip_connections) != [1]
            or not (head.hidden_dims == 64 if width == WIDTH_64 else head.hidden_dims % 4 == 0)):
        return None
    lw = tuple(p for l in head.layers for p in (l.weight, l.bias))
    return None if any(p is None for p in lw) else lw


def timestamps_of(data_dict) -> Optional[Tensor]:
    return data_dict["normed_timestamps"] if "normed_timestamps" in data_dict else data_dict.get("lidar_normed_timestamps")


def appearance_key(cam_embedding: bool, img_embedding: bool, data_dict) -> Optional[str]:
    """The entry of data_dict that indexes the appearance embedding, or None (no embedding, or no index: the mean embedding, :641-643)."""
    if cam_embedding and "cam_idx" in data_dict:
        return "cam_idx"
    return "img_idx" if (img_embedding and "img_idx" in data_dict) else None


# ------------------------------------------------------------------ the flow pair: one writer, one reader
_FLOW_PAIR_CARRIER = "forward_pred_backward_flow"


def attach_flow_pair(results: Dict[str, Tensor], flow: Tensor, flow2: Tensor) -> None:
    """[r5] The cycle loss reads its four operands as column blocks of the flow MLP's two outputs (ops.reg_losses(flow_pair=...)).  The
    result keys stay the reference's, so the pair rides as an attribute of one of the four views: render_utils._extras hands it on."""
    results[_FLOW_PAIR_CARRIER]._emer_flow_pair = (flow, flow2)


def flow_pair(extras: Dict[str, Tensor]) -> Optional[Tuple[Tensor, Tensor]]:
    """(flow [.., 6], flow2 [2N, 6]) of the batched flow branch, or None (another route, or the carrier was re-made on the way)."""
    return getattr(extras.get(_FLOW_PAIR_CARRIER), "_emer_flow_pair", None)


class _EmbedFn(torch.autograd.Function):
    """nn.Embedding lookup whose backward is ONE index_add (atomic scatter) instead of torch's sort + segmented-reduce
    pipeline (~20 launches for 8192 rays); same values up to fp32 summation order."""

    @staticmethod
    def forward(ctx, weight: Tensor, idx: Tensor):
        ctx.save_for_backward(idx)
        ctx.shape = weight.shape
        return weight.index_select(0, idx.reshape(-1)).view(*idx.shape, weight.shape[1])

    @staticmethod
    def backward(ctx, g: Tensor):
        (idx,) = ctx.saved_tensors
        dw = torch.zeros(ctx.shape, device=g.device, dtype=g.dtype)
        dw.index_add_(0, idx.reshape(-1), g.reshape(-1, ctx.shape[1]))
        return dw, None


class _ForwardCache:
    """The rgb head and the sky head of one forward look up the SAME per-ray indices (:637-643, 668-674): the second use takes the first
    one's result (one gather / one launch forward, one scatter backward; autograd sums the two gradients).  Two slots of one (key, value)
    each; a key names storages, versions and the grad mode, so no slot serves a stale value; RadianceField.forward clears both on entry."""

    def __init__(self):
        self.embedding = self.ray_rows = None   # _EmbedFn per ray | the rows of fused.ray_inputs

    clear = __init__

    def __reduce__(self):   # copies and pickles of a model start empty (the entries are graph tensors of one forward)
        return _ForwardCache, ()

    def get(self, slot: str, make: Callable, *tensors: Tensor):
        key = (torch.is_grad_enabled(), *((t.data_ptr(), t._version, t.shape, t.stride()) for t in tensors))
        hit = getattr(self, slot)
        if hit is None or hit[0] != key:
            hit = (key, make(*tensors))
            setattr(self, slot, hit)
        return hit[1]


class MLP(nn.Module):
    """radiance_fields/mlp.py:7-46 (skip-connection MLP of the rgb / sky heads)."""

    def __init__(self, in_dims: int, out_dims: int, num_layers: int = 3, hidden_dims: Optional[int] = 256,
                 skip_connections: Optional[Tuple[int]] = [0]) -> None:
        super().__init__()
        self.in_dims, self.hidden_dims, self.n_output_dims = in_dims, hidden_dims, out_dims
        self.num_layers, self.skip_connections = num_layers, skip_connections
        layers = []
        if num_layers == 1:
            layers.append(nn.Linear(in_dims, out_dims))
        else:
            for i in range(num_layers - 1):
                if i == 0:
                    layers.append(nn.Linear(in_dims, hidden_dims))
                elif i in skip_connections:
                    layers.append(nn.Linear(in_dims + hidden_dims, hidden_dims))
                else:
                    layers.append(nn.Linear(hidden_dims, hidden_dims))
            layers.append(nn.Linear(hidden_dims, out_dims))
        self.layers = nn.ModuleList(layers)

    def forward(self, x: Tensor, final_act: Optional[str] = None) -> Tensor:
        inp = x
        n = len(self.layers)
        for i, layer in enumerate(self.layers):
            if i in self.skip_connections:
                x = torch.cat([x, inp], -1)
            x = ops.linear(x, layer.weight, layer.bias, "relu" if i < n - 1 else final_act)
        return x


def _as_box(aabb: Union[Tensor, List[float]]) -> Tensor:
    return aabb if isinstance(aabb, Tensor) else torch.tensor(aabb, dtype=torch.float32)


class _Boxed(nn.Module):
    """A field inside an axis-aligned box: the ``aabb`` buffer (the first entry of the state dict), ``set_aabb`` and ``device``."""
    _box_name = "aabb"

    def __init__(self, aabb: Union[Tensor, List[float]], density_activation: Optional[Callable]) -> None:
        super().__init__()
        if density_activation is not None:
            raise NotImplementedError("only the reference's default density activation trunc_exp(x - 1) is fused")
        self.register_buffer("aabb", _as_box(aabb))

    def set_aabb(self, aabb: Union[Tensor, List[float]]) -> None:
        aabb = _as_box(aabb)
        logger.info(f"Set {self._box_name} from {self.aabb} to {aabb}")
        self.aabb.copy_(aabb)
        self.aabb = self.aabb.to(self.device)

    @property
    def device(self) -> torch.device:
        return self.aabb.device


class _Dynamic(NamedTuple):
    """What the dynamic branch of a forward hands back, whichever route computed it."""
    geo: Tensor                 # geometry features [..., 64 or geometry_feature_dim]
    sem: Optional[Tensor]       # semantic features, None when the model has none
    density: Tensor
    extras: Dict[str, Tensor]   # the flow branch's entries of the result dictionary, in the reference's order


FUSE_FLOW_WARP = True  # ... and build its warped xyzt query points (and their gradient) in one launch each way (ops.flow_warp) [r4]
BATCH_XYZT = True  # flow configs: evaluate each xyzt table once per dependency level (RadianceField._flow_branch)
FUSE_FIELD = os.environ.get("EMER_FUSE_FIELD", "1") != "0"   # neck + rgb head of the static model as one forward launch (fused.RgbRider); 0: two launches


class RadianceField(_Boxed):
    """radiance_fields/radiance_field.py:20-785."""

    def __init__(
        self,
        xyz_encoder: HashEncoder,
        dynamic_xyz_encoder: Optional[HashEncoder] = None,
        flow_xyz_encoder: Optional[HashEncoder] = None,
        aabb: Union[Tensor, List[float]] = [-1, -1, -1, 1, 1, 1],
        num_dims: int = 3,
        density_activation: Optional[Callable] = None,
        unbounded: bool = True,
        geometry_feature_dim: int = 15,
        base_mlp_layer_width: int = 64,
        head_mlp_layer_width: int = 64,
        enable_cam_embedding: bool = False,
        enable_img_embedding: bool = False,
        num_cams: int = 3,
        appearance_embedding_dim: int = 16,
        semantic_feature_dim: int = 64,
        feature_mlp_layer_width: int = 256,
        feature_embedding_dim: int = 768,
        enable_sky_head: bool = False,
        enable_shadow_head: bool = False,
        enable_feature_head: bool = False,
        num_train_timesteps: int = 0,
        interpolate_xyz_encoding: bool = False,
        enable_learnable_pe: bool = True,
        enable_temporal_interpolation: bool = False,
    ) -> None:
        super().__init__(aabb, density_activation)
        self.unbounded, self.num_cams, self.num_dims = unbounded, num_cams, num_dims
        self.enable_cam_embedding, self.enable_img_embedding = enable_cam_embedding, enable_img_embedding
        self.appearance_embedding_dim = appearance_embedding_dim
        self.geometry_feature_dim = geometry_feature_dim
        if not enable_feature_head:
            semantic_feature_dim = 0
        self.semantic_feature_dim = semantic_feature_dim

        # ---- static field (radiance_field.py:72-80)
        self.xyz_encoder = xyz_encoder
        self.base_mlp = nn.Sequential(
            nn.Linear(self.xyz_encoder.n_output_dims, base_mlp_layer_width), nn.ReLU(),
            nn.Linear(base_mlp_layer_width, geometry_feature_dim + semantic_feature_dim))
        # ---- dynamic field (:82-96)
        self.interpolate_xyz_encoding = interpolate_xyz_encoding
        self.dynamic_xyz_encoder = dynamic_xyz_encoder
        self.enable_temporal_interpolation = enable_temporal_interpolation
        if self.dynamic_xyz_encoder is not None:
            self.register_buffer("training_timesteps", torch.zeros(num_train_timesteps))
            self.dynamic_base_mlp = nn.Sequential(
                nn.Linear(self.dynamic_xyz_encoder.n_output_dims, base_mlp_layer_width), nn.ReLU(),
                nn.Linear(base_mlp_layer_width, geometry_feature_dim + semantic_feature_dim))
        # ---- flow field (:98-111)
        self.flow_xyz_encoder = flow_xyz_encoder
        if self.flow_xyz_encoder is not None:
            self.flow_mlp = nn.Sequential(
                nn.Linear(self.flow_xyz_encoder.n_output_dims, base_mlp_layer_width), nn.ReLU(),
                nn.Linear(base_mlp_layer_width, base_mlp_layer_width), nn.ReLU(),
                nn.Linear(base_mlp_layer_width, 6))
        # ---- appearance embedding (:113-123)
        if self.enable_cam_embedding:
            self.appearance_embedding = nn.Embedding(num_cams, appearance_embedding_dim)
        elif self.enable_img_embedding:
            self.appearance_embedding = nn.Embedding(num_train_timesteps * num_cams, appearance_embedding_dim)
        else:
            self.appearance_embedding = None
        self.direction_encoding = SinusoidalEncoder(n_input_dims=3, min_deg=0, max_deg=4)
        emb = appearance_embedding_dim if (enable_cam_embedding or enable_img_embedding) else 0
        # ---- colour head (:130-143)
        self.rgb_head = MLP(in_dims=geometry_feature_dim + self.direction_encoding.n_output_dims + emb, out_dims=3,
                            num_layers=3, hidden_dims=head_mlp_layer_width, skip_connections=[1])
        # ---- shadow head (:145-153)
        self.enable_shadow_head = enable_shadow_head
        if enable_shadow_head:
            self.shadow_head = nn.Sequential(nn.Linear(geometry_feature_dim, base_mlp_layer_width), nn.ReLU(),
                                             nn.Linear(base_mlp_layer_width, 1), nn.Sigmoid())
        # ---- sky heads (:155-187)
        self.enable_sky_head = enable_sky_head
        if enable_sky_head:
            self.sky_head = MLP(in_dims=self.direction_encoding.n_output_dims + emb, out_dims=3, num_layers=3,
                                hidden_dims=head_mlp_layer_width, skip_connections=[1])
            if enable_feature_head:
                self.dino_sky_head = nn.Sequential(
                    nn.Linear(self.direction_encoding.n_output_dims + emb, feature_mlp_layer_width), nn.ReLU(),
                    nn.Linear(feature_mlp_layer_width, feature_mlp_layer_width), nn.ReLU(),
                    nn.Linear(feature_mlp_layer_width, feature_embedding_dim))
        # ---- feature head (:189-217)
        self.enable_feature_head = enable_feature_head
        if enable_feature_head:
            self.dino_head = nn.Sequential(
                nn.Linear(semantic_feature_dim, feature_mlp_layer_width), nn.ReLU(),
                nn.Linear(feature_mlp_layer_width, feature_mlp_layer_width), nn.ReLU(),
                nn.Linear(feature_mlp_layer_width, feature_embedding_dim))
            self.register_buffer("feats_reduction_mat", torch.zeros(feature_embedding_dim, 3))
            self.register_buffer("feat_color_min", torch.zeros(3, dtype=torch.float32))
            self.register_buffer("feat_color_max", torch.ones(3, dtype=torch.float32))
            self.enable_learnable_pe = enable_learnable_pe
            if enable_learnable_pe:
                self.learnable_pe_map = nn.Parameter(0.05 * torch.randn(1, feature_embedding_dim // 2, 80, 120), requires_grad=True)
                self.pe_head = nn.Sequential(nn.Linear(feature_embedding_dim // 2, feature_embedding_dim))
        self.time_diff = 0
        self._time_diff_read = (None, 0.0)   # (the object ``time_diff`` was when it was last read, its float)
        self._cache = _ForwardCache()
        self.last_routes: Dict[str, str] = {}

    # ------------------------------------------------------------------ bookkeeping (:219-276)
    def register_normalized_training_timesteps(self, normalized_timesteps: Tensor, time_diff: float = None) -> None:
        if self.dynamic_xyz_encoder is not None:
            self.training_timesteps.copy_(normalized_timesteps)
            self.training_timesteps = self.training_timesteps.to(self.device)
            if time_diff is not None:
                self.time_diff = time_diff
            elif len(self.training_timesteps) > 1:
                self.time_diff = self.training_timesteps[1] - self.training_timesteps[0]
            else:
                self.time_diff = 0
            self._time_diff_float()   # read back here, outside any graph capture, so that the default registration takes the fused warp too

    def _time_diff_float(self) -> float:
        """``time_diff`` (a 0-dim tensor on the reference's default route) as the kernel argument of the one-launch flow warp: ONE host
        read per object it is bound to, at the registration or at the first use after a direct assignment, never during a later capture."""
        if self._time_diff_read[0] is not self.time_diff:
            self._time_diff_read = (self.time_diff, float(self.time_diff))
        return self._time_diff_read[1]

    def register_feats_reduction_mat(self, feats_reduction_mat: Tensor, feat_color_min: Tensor, feat_color_max: Tensor) -> None:
        self.feats_reduction_mat.copy_(feats_reduction_mat)
        self.feat_color_min.copy_(feat_color_min)
        self.feat_color_max.copy_(feat_color_max)

    # ------------------------------------------------------------------ routes (the table in the module docstring)
    def _neck_ok(self, encoder: HashEncoder, mlp: nn.Sequential) -> bool:
        d = encoder.tcnn_encoding.desc
        return neck_eligible(self.geometry_feature_dim, self.semantic_feature_dim, d.n_levels, d.n_features,
                             mlp[0].out_features, mlp[2].out_features)

    def _dynamic_route(self, want_hash: bool) -> str:
        return "neck" if self._neck_ok(self.dynamic_xyz_encoder, self.dynamic_base_mlp) else ("sequential" if want_hash else "chain")

    def _flow_mlp_params(self):
        return tuple([getattr(m, p) for m in self.flow_mlp if isinstance(m, nn.Linear)] for p in ("weight", "bias"))

    def _flow_routes(self) -> Dict[str, str]:
        """The routes of one flow-field evaluation (forward_flow_hash called directly)."""
        d = self.flow_xyz_encoder.tcnn_encoding.desc
        return {"flow": "interpolated" if (self.enable_temporal_interpolation and not self.training) else "call_by_call",
                "flow_mlp": "fused" if flow_mlp_eligible(*self._flow_mlp_params(), d.n_levels, d.n_features) else "sequential"}

    def _appearance_key(self, data_dict) -> Optional[str]:
        return appearance_key(self.enable_cam_embedding, self.enable_img_embedding, data_dict or {})

    def _rgb_route(self, directions: Tensor, data_dict, rows: bool, rider_ok: bool = False) -> str:
        """rows: _ray_rows_args(directions, data_dict) is not None; rider_ok: the static neck of this forward can carry a rider."""
        key = self._appearance_key(data_dict)
        if not (directions.dim() == 3 and self._per_ray(directions) and (rows or key is None or self._per_ray(data_dict[key]))
                and skip_head_params(self.rgb_head, WIDTH_CHAIN) is not None):
            return "general"
        return "rider" if (rider_ok and FUSE_FIELD and rows and skip_head_params(self.rgb_head, WIDTH_64) is not None) else "per_ray"

    def _sky_route(self) -> str:
        return "ray_chain" if skip_head_params(self.sky_head, WIDTH_CHAIN) is not None else "module"

    def _routes(self, positions, normed_positions, directions, data_dict, return_density_only: bool) -> Dict[str, str]:
        r = dict.fromkeys(("static", "dynamic", "flow", "flow_mlp", "warp", "rgb", "sky", "ray_inputs"), "none")
        r["static"] = "neck" if self._neck_ok(self.xyz_encoder, self.base_mlp) else "chain"
        ts = timestamps_of(data_dict)
        if self.dynamic_xyz_encoder is not None and ts is not None:
            use_flow = self.flow_xyz_encoder is not None
            r["dynamic"] = self._dynamic_route(want_hash=use_flow)
            if use_flow:
                r.update(self._flow_routes())
                if (r["flow"] != "interpolated" and BATCH_XYZT and positions is not None and r["dynamic"] == "neck"
                        and r["flow_mlp"] == "fused"):
                    r["flow"] = "batched"
                    # (the current xyzt points carry no gradient in a training step: inputs of the model)
                    x_grad = torch.is_grad_enabled() and (normed_positions.requires_grad or ts.requires_grad)
                    r["warp"] = "fused" if (FUSE_FLOW_WARP and self.num_dims == 3 and not positions.requires_grad and not x_grad) else "torch"
        if not return_density_only and directions is not None:
            rows = self._ray_rows_args(directions, data_dict) is not None
            r["rgb"] = self._rgb_route(directions, data_dict, rows, rider_ok=r["static"] == "neck" and normed_positions.dim() == 3)
            if self.enable_sky_head and "lidar_origin" not in data_dict:
                r["sky"] = self._sky_route()
            r["ray_inputs"] = "shared" if rows else "separate"
        return r

    # ------------------------------------------------------------------ field pieces
    def contract_points(self, positions: Tensor) -> Tensor:
        """:278-300 (contraction + selector zeroing), one fused kernel, differentiable."""
        return ops.contract_points(positions, self.aabb, self.unbounded)

    def _base(self, encoder: HashEncoder, mlp: nn.Sequential, x: Tensor):
        """grid -> Linear-ReLU-Linear (+ density of feature 0): one level-major grid kernel + one fused chain."""
        enc_lm = encoder.tcnn_encoding.forward_level_major(x)
        return fused.base_mlp(enc_lm, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)

    def _neck(self, encoder: HashEncoder, mlp: nn.Sequential, x: Tensor, rider=None):
        """Route "neck" on rows x [N, D] -> (geo, sem or None, density, the level-major encoding): the register-resident kernel writes the
        two halves as separate [N, 64] tensors -- the split of :400 costs nothing and an unused semantic half gets no backward work."""
        enc_lm = encoder.tcnn_encoding.forward_level_major(x)
        # the rider is built AFTER the encode: its per-ray input node must be younger than the grid node, so that autograd
        # runs the embedding gradient BEFORE the table backward (the data-parallel early bucket relies on the static
        # table's backward being the last writer of the step, trainer.py)
        rider = rider() if callable(rider) else rider
        return (*fused.neck(enc_lm, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias, rider=rider), enc_lm)

    def _split_feats(self, encoder: HashEncoder, mlp: nn.Sequential, x: Tensor, route: str, rider=None):
        """(geo feats, semantic feats or None, density) of a grid + neck at the points x [..., D] by route "neck" or "chain"."""
        lead = x.shape[:-1]
        if route == "neck":
            geo, sem, density, _ = self._neck(encoder, mlp, x.reshape(-1, x.shape[-1]), rider)
        else:
            feats, density = self._base(encoder, mlp, x.reshape(-1, x.shape[-1]))
            geo, sem = torch.split(feats, [self.geometry_feature_dim, self.semantic_feature_dim], dim=-1)
        return geo.view(*lead, -1), (None if sem is None else sem.view(*lead, -1)), density.view(*lead)

    def forward_static_hash(self, positions: Tensor) -> Tuple[Tensor, Tensor]:
        """:302-318.  Returns (encoded_features, normed_positions)."""
        normed_positions = self.contract_points(positions)
        feats, _ = self._base(self.xyz_encoder, self.base_mlp, normed_positions.reshape(-1, self.num_dims))
        return feats.view(*normed_positions.shape[:-1], -1), normed_positions

    @staticmethod
    def _xyzt(normed_positions: Tensor, normed_timestamps: Tensor) -> Tensor:
        if normed_timestamps.shape[-1] != 1:
            normed_timestamps = normed_timestamps.unsqueeze(-1)
        return torch.cat([normed_positions, normed_timestamps.to(normed_positions.dtype)], dim=-1)

    def forward_dynamic_hash(self, normed_positions: Tensor, normed_timestamps: Tensor, return_hash_encodings: bool = False,
                             _route: Optional[str] = None):
        """:320-357 (the ``if True:`` branch: no temporal interpolation), with the row-major hash encodings of :457-459, 615-617."""
        x = self._xyzt(normed_positions, normed_timestamps)
        lead, x = x.shape[:-1], x.reshape(-1, self.num_dims + 1)
        if (_route or self._dynamic_route(want_hash=True)) == "neck":
            # level-major encoding -> register-resident neck; the hash encodings are one transpose of the same tensor, not a
            # second path through the MLP
            geo, sem, _, enc_lm = self._neck(self.dynamic_xyz_encoder, self.dynamic_base_mlp, x)
            feats = geo if sem is None else torch.cat([geo, sem], dim=-1)
            enc = ops.lm_to_rm(enc_lm)
        else:   # "sequential"
            enc = self.dynamic_xyz_encoder(x)
            feats = _run_sequential(self.dynamic_base_mlp, enc)
        feats, enc = feats.view(*lead, -1), enc.view(*lead, -1)
        return (feats, enc) if return_hash_encodings else feats

    def forward_flow_hash(self, normed_positions: Tensor, normed_timestamps: Tensor, _routes: Optional[Dict[str, str]] = None) -> Tensor:
        """:359-389.  Evaluation with ``enable_temporal_interpolation``: the flow field BETWEEN two training timesteps is the flow
        MLP of the linearly interpolated xyzt encodings at the two nearest training timesteps (``temporal_interpolation``, :844-905,
        called with interpolate_xyz_encoding=True).  (The dynamic branch never interpolates: the reference's ``if True:``, :336-337.)"""
        routes = _routes or self._flow_routes()
        if normed_timestamps.shape[-1] != 1:
            normed_timestamps = normed_timestamps.unsqueeze(-1)
        if routes["flow"] == "interpolated":
            return self._flow_hash_interpolated(normed_positions, normed_timestamps, routes["flow_mlp"])
        return self._flow_from_xyzt(self._xyzt(normed_positions, normed_timestamps), routes["flow_mlp"])

    def _flow_hash_interpolated(self, normed_positions: Tensor, normed_timestamps: Tensor, mlp_route: str) -> Tensor:
        """temporal_interpolation (:844-905) for the flow encoder.  One timestamp per ray (the slice [:, 0(, 0)] the reference reads);
        when EVERY ray sits on a training timestep the plain evaluation is used (its ``torch.allclose`` test: one host read, eval only)."""
        slice_t = normed_timestamps[:, 0] if normed_timestamps.dim() == 2 else normed_timestamps[:, 0, 0]
        train_t = self.training_timesteps.to(slice_t)
        # find_topk_nearby_timesteps (nerf_utils.py:31-57): the two training timesteps closest to each query
        idx = torch.topk((train_t[None, :] - slice_t[:, None]).abs(), k=2, dim=1, largest=False).indices
        closest = train_t[idx]
        if torch.allclose(closest[:, 0], slice_t):
            return self._flow_from_xyzt(self._xyzt(normed_positions, normed_timestamps), mlp_route)
        assert normed_positions.dim() == 3, "temporal interpolation expects (rays, samples, 3) positions, as the reference does"
        S = normed_positions.shape[1]
        left, right = closest[:, 0], closest[:, 1]
        offset = ((slice_t - left) / (right - left))[:, None, None]
        enc = self.flow_xyz_encoder
        xl = torch.cat([normed_positions, left[:, None, None].expand(-1, S, 1)], dim=-1)
        xr = torch.cat([normed_positions, right[:, None, None].expand(-1, S, 1)], dim=-1)
        el = enc(xl.reshape(-1, self.num_dims + 1)).view(*xl.shape[:-1], -1)
        er = enc(xr.reshape(-1, self.num_dims + 1)).view(*xr.shape[:-1], -1)
        return _run_sequential(self.flow_mlp, el * (1 - offset) + er * offset)

    def _flow_from_xyzt(self, temporal_positions: Tensor, mlp_route: str) -> Tensor:
        x = temporal_positions.reshape(-1, self.num_dims + 1)
        if mlp_route == "fused":
            # level-major xyzt encoding straight into the register-resident 3-layer MLP (no row-major copy either way)
            flow = fused.seq_mlp_lm(self.flow_xyz_encoder.tcnn_encoding.forward_level_major(x), *self._flow_mlp_params())
        else:
            flow = _run_sequential(self.flow_mlp, self.flow_xyz_encoder(x))
        return flow.view(*temporal_positions.shape[:-1], 6)

    def _noise(self, like: Tensor) -> Tensor:
        """Temporal-aggregation noise (:567-570); overridable so tests can replay the reference's draw."""
        if self.training:
            return torch.rand_like(like)[..., 0:1]
        return torch.ones_like(like)[..., 0:1]

    def _warp(self, positions: Tensor, ts: Tensor, forward_flow: Tensor, backward_flow: Tensor, noise: Tensor):
        """The points one (noisy) time step ahead and behind (:567-580): (forward xyz, backward xyz, forward t, backward t)."""
        return (self.contract_points(positions + forward_flow * noise), self.contract_points(positions + backward_flow * noise),
                torch.clamp(ts + self.time_diff * noise, 0, 1.0), torch.clamp(ts - self.time_diff * noise, 0, 1.0))

    def temporal_aggregation(self, positions: Tensor, normed_timestamps: Tensor, forward_flow: Tensor,
                             backward_flow: Tensor, dynamic_feats: Tensor, _routes: Optional[Dict[str, str]] = None) -> Dict[str, Tensor]:
        """:553-620 (Eq. 8 of the paper)."""
        routes = _routes or dict(self._flow_routes(), dynamic=self._dynamic_route(want_hash=True))
        if normed_timestamps.shape[-1] != 1:
            normed_timestamps = normed_timestamps.unsqueeze(-1)
        noise = self._noise(forward_flow)
        fwd_pos, bwd_pos, fwd_t, bwd_t = self._warp(positions, normed_timestamps, forward_flow, backward_flow, noise)
        fwd_feats, fwd_enc = self.forward_dynamic_hash(fwd_pos, fwd_t, return_hash_encodings=True, _route=routes["dynamic"])
        bwd_feats, bwd_enc = self.forward_dynamic_hash(bwd_pos, bwd_t, return_hash_encodings=True, _route=routes["dynamic"])
        fwd_pred_flow = self.forward_flow_hash(fwd_pos, fwd_t, routes)
        bwd_pred_flow = self.forward_flow_hash(bwd_pos, bwd_t, routes)
        aggregated = (dynamic_feats + 0.5 * fwd_feats + 0.5 * bwd_feats) / 2.0
        return {
            "dynamic_feats": aggregated,
            "forward_pred_backward_flow": fwd_pred_flow[..., 3:],
            "backward_pred_forward_flow": bwd_pred_flow[..., :3],
            "forward_dynamic_hash_encodings": fwd_enc,
            "backward_dynamic_hash_encodings": bwd_enc,
        }

    def _flow_branch(self, positions: Tensor, normed_positions: Tensor, normed_timestamps: Tensor, want_hash: bool,
                     warp_route: str) -> _Dynamic:
        """Route "batched" of the flow branch (:434-459 + temporal_aggregation :553-620), every xyzt table in as few launches as the data
        flow allows: the flow grid at the current positions (N samples) -> flow MLP -> warped positions -> the dynamic grid ONCE at
        [current | forward-warped | backward-warped] (3N samples: one encode, one neck, one owner-computes backward) and the flow grid
        ONCE at both warped sets (2N).  Six encodes / six table backwards / four input-gradient launches of the call-by-call order become
        3 / 3 / 2, and each table's slices are flushed once per step, not three times.  Same arithmetic per sample."""
        enc_d, enc_f = self.dynamic_xyz_encoder.tcnn_encoding, self.flow_xyz_encoder.tcnn_encoding
        mlp = self.dynamic_base_mlp
        if normed_timestamps.shape[-1] != 1:
            normed_timestamps = normed_timestamps.unsqueeze(-1)
        lead = normed_positions.shape[:-1]
        D4 = self.num_dims + 1
        ts = normed_timestamps.to(normed_positions.dtype)
        x_cur = torch.cat([normed_positions, ts], dim=-1).reshape(-1, D4)
        N = x_cur.shape[0]
        fw, fb = self._flow_mlp_params()
        # (1) flow at the current positions
        flow = fused.seq_mlp_lm(enc_f.forward_level_major(x_cur), fw, fb).view(*lead, 6)
        forward_flow, backward_flow = flow[..., :3], flow[..., 3:]
        # (2) warped positions and times (:567-580)
        noise = self._noise(forward_flow)
        if warp_route == "fused":
            # [r4] one launch for both warps, both clamps and the batch assembly (and one for their gradient w.r.t. the flow), instead
            # of 14 elementwise / cat launches and ~18 autograd twins; the flow table's 2N-row batch is a second output, so the two
            # tables' input gradients arrive as two tensors (no pad / copy / add)
            if noise.requires_grad:   # (only a _noise override can do that)
                raise ValueError("ops.flow_warp takes the aggregation noise as a constant: set radiance_field.FUSE_FLOW_WARP = False")
            x3, x2 = ops.flow_warp(positions, normed_positions, ts, flow, noise, self._time_diff_float(), self.aabb, self.unbounded)
        else:
            fwd_pos, bwd_pos, fwd_t, bwd_t = self._warp(positions, ts, forward_flow, backward_flow, noise)
            x_fwd = torch.cat([fwd_pos, fwd_t.to(fwd_pos.dtype)], dim=-1).reshape(-1, D4)
            x_bwd = torch.cat([bwd_pos, bwd_t.to(bwd_pos.dtype)], dim=-1).reshape(-1, D4)
            x3, x2 = torch.cat([x_cur, x_fwd, x_bwd], dim=0), torch.cat([x_fwd, x_bwd], dim=0)
        # (3) dynamic table: one evaluation of 3N samples, one neck
        # the current positions carry no gradient in a training step (inputs of the model); a caller that asks for one gets it
        enc3 = enc_d.forward_level_major(x3, skip_dx_rows=0 if x_cur.requires_grad else N)
        geo3, sem3, _ = fused.neck(enc3, mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)
        # temporal aggregation (:595-613) per feature half, straight from the 3N-row batch: one launch each way, no [., 128]
        # concatenation and no 3N-row cat in the backward; [r4] the density (trunc_exp of the aggregated geometry features'
        # column 0, :461) comes out of the same launch
        geo, density = ops.aggregate3_density(geo3)
        geo, density = geo.view(*lead, -1), density.view(*lead)
        sem = None if sem3 is None else ops.aggregate3(sem3).view(*lead, -1)
        # (4) flow table at both warped sets: one evaluation of 2N samples
        flow2 = fused.seq_mlp_lm(enc_f.forward_level_major(x2), fw, fb)
        fwd_pred, bwd_pred = (t.view(*lead, 6) for t in flow2.split(N, dim=0))
        out = {"forward_flow": forward_flow, "backward_flow": backward_flow, "dynamic_feats": geo,
               "forward_pred_backward_flow": fwd_pred[..., 3:], "backward_pred_forward_flow": bwd_pred[..., :3]}
        attach_flow_pair(out, flow, flow2)
        if want_hash:  # row-major copies of the encodings: part of forward()'s contract (:453-459, 615-617), consumed by nobody
            cur_h, fwd_h, bwd_h = (t.view(*lead, -1) for t in ops.lm_to_rm(enc3).split(N, dim=0))
            out.update({"forward_dynamic_hash_encodings": fwd_h, "backward_dynamic_hash_encodings": bwd_h,
                        "current_dynamic_hash_encodings": cur_h})
        if sem is not None:   # the halves stay apart: the reference's [., 128] tensor on request only
            if want_hash:
                out["dynamic_feats"] = torch.cat([geo, sem], dim=-1)
            else:
                del out["dynamic_feats"]
        return _Dynamic(geo, sem, density, out)

    def _flow_call_by_call(self, positions: Tensor, normed_positions: Tensor, normed_timestamps: Tensor, routes: Dict[str, str]) -> _Dynamic:
        """Routes "call_by_call" and "interpolated" of the flow branch: the reference's order of calls (:434-461)."""
        feats, enc = self.forward_dynamic_hash(normed_positions, normed_timestamps, return_hash_encodings=True, _route=routes["dynamic"])
        flow = self.forward_flow_hash(normed_positions, normed_timestamps, routes)
        out = {"forward_flow": flow[..., :3], "backward_flow": flow[..., 3:]}
        out.update(self.temporal_aggregation(positions, normed_timestamps, out["forward_flow"], out["backward_flow"], feats, routes))
        out["current_dynamic_hash_encodings"] = enc
        feats = out["dynamic_feats"]
        density = ops.trunc_exp_column(feats, 0)
        if self.semantic_feature_dim == 0:
            # (torch.split(x, [64, 0]) is a view forward and a full-size cat backward -- 31 us per flow step for an empty half)
            return _Dynamic(feats, None, density, out)
        return _Dynamic(*torch.split(feats, [self.geometry_feature_dim, self.semantic_feature_dim], dim=-1), density, out)

    @staticmethod
    def _per_ray(t: Tensor) -> bool:
        """True for a (R, S[, C]) tensor that is a stride-0 broadcast of per-ray values along S (what
        render_rays passes instead of the reference's repeat_interleave copies)."""
        return t.dim() >= 2 and t.shape[1] > 1 and t.stride(1) == 0

    def _embed(self, idx: Tensor) -> Tensor:
        if self._per_ray(idx):  # look up once per ray, broadcast along the samples (same values, 1/S of the work)
            return self._cache.get("embedding", _EmbedFn.apply, self.appearance_embedding.weight, idx[:, 0])[:, None, :].expand(-1, idx.shape[1], -1)
        if idx.dim() == 1:  # the sky head's per-ray indices: the same storage the rgb head just looked up
            return self._cache.get("embedding", _EmbedFn.apply, self.appearance_embedding.weight, idx)
        return _EmbedFn.apply(self.appearance_embedding.weight, idx)

    def _encode_dirs(self, directions: Tensor, remap: bool) -> Tensor:
        if self._per_ray(directions):
            enc = self.direction_encoding(directions[:, 0].contiguous(), remap=remap)
            return enc[:, None, :].expand(-1, directions.shape[1], -1)
        return self.direction_encoding(directions, remap=remap)

    def _appearance(self, directions: Tensor, data_dict: Optional[Dict[str, Tensor]]):
        if self.appearance_embedding is None:
            return None
        key = self._appearance_key(data_dict)
        if key is not None:
            return self._embed(data_dict[key])
        return torch.ones((*directions.shape[:-1], self.appearance_embedding_dim), device=directions.device) \
            * self.appearance_embedding.weight.mean(dim=0)

    def _ray_rows_args(self, directions: Optional[Tensor], data_dict: Optional[Dict[str, Tensor]]):
        """(embedding weight, per-ray indices [R], per-ray directions [R, 3]) that fused.ray_inputs takes, or None when the inputs
        are not per-ray / there is no embedding index (then the heads build their inputs separately).  Views only, no launch."""
        key = self._appearance_key(data_dict)
        if key is None or directions is None:
            return None
        idx = data_dict[key]
        idx = idx[:, 0] if self._per_ray(idx) else idx
        d = directions[:, 0] if (directions.dim() == 3 and self._per_ray(directions)) else directions
        enc = self.direction_encoding
        if not (idx.dim() == 1 and d.dim() == 2 and d.shape[0] == idx.shape[0] and idx.dtype == torch.int64 and d.is_cuda
                and d.dtype == torch.float32 and d.stride(1) == 1 and not d.requires_grad
                and enc.n_input_dims == 3 and enc.min_deg == 0 and enc.enable_identity):
            return None
        return self.appearance_embedding.weight, idx, d

    def _ray_inputs(self, directions: Tensor, data_dict: Optional[Dict[str, Tensor]]):
        """(rgb-head rows, sky-head rows) = [direction PE | appearance embedding] per RAY from one launch, shared by the two heads of a
        forward pass (they look up the same indices, :637-643 and :668-674), or None (see _ray_rows_args).  ``front``: the launch also
        evaluates the per-ray stages of the two heads that consume the rows, where they are 64 wide; they check again what they pick up."""
        args = self._ray_rows_args(directions, data_dict)
        if args is None:
            return None
        front = lambda: (skip_head_params(self.rgb_head, WIDTH_64), skip_head_params(getattr(self, "sky_head", None), WIDTH_64), fused.ACT_SIGMOID)
        return self._cache.get("ray_rows", lambda w, idx, d: fused.ray_inputs(w, idx, d, self.direction_encoding.max_deg, front=front()), *args)

    def _rgb_per_ray(self, directions, data_dict) -> Callable:
        """Routes "per_ray" and "rider", as a function of the geometry features: per-ray [dir-PE | appearance emb] stays per ray, geo stays per sample, the whole
        3-layer skip MLP + sigmoid is one chain (fused.rgb_head; a head too wide for one chain launch -- fused.rgb_head_supported,
        e.g. 128 or 256 hidden units -- runs layer by layer there).  Applies when render_rays hands in stride-0 per-ray views."""
        R, S = directions.shape[:2]
        both = self._ray_inputs(directions, data_dict)
        if both is not None:
            hray = both[0]
        else:
            emb = None
            if self.appearance_embedding is not None:
                key = self._appearance_key(data_dict)
                emb = self.appearance_embedding.weight.mean(dim=0)[None, :].expand(R, -1) if key is None else \
                    self._cache.get("embedding", _EmbedFn.apply, self.appearance_embedding.weight, data_dict[key][:, 0])
            pe = self.direction_encoding(directions[:, 0].contiguous(), remap=True)
            hray = pe if emb is None else torch.cat([pe, emb], dim=-1)
        lw = skip_head_params(self.rgb_head, WIDTH_CHAIN)

        def run(geo):
            g2 = geo.reshape(R * S, geo.shape[-1])
            if g2.stride(-1) != 1:
                g2 = g2.contiguous()
            return fused.rgb_head(hray, g2, S, *lw).view(R, S, -1)
        return run

    def query_rgb(self, directions: Tensor, geo_feats: Tensor, dynamic_geo_feats: Tensor = None,
                  data_dict: Dict[str, Tensor] = None, _route: Optional[str] = None) -> Dict[str, Tensor]:
        """:622-658."""
        route = _route or self._rgb_route(directions, data_dict, self._ray_rows_args(directions, data_dict) is not None)
        if route != "general":
            run = self._rgb_per_ray(directions, data_dict)
        else:
            h = self._encode_dirs(directions, remap=True)  # (d + 1) / 2 folded into the kernel
            emb = self._appearance(directions, data_dict)
            if emb is not None:
                h = torch.cat([h, emb], dim=-1)
            run = lambda geo: self.rgb_head(torch.cat([h, geo], dim=-1), final_act="sigmoid")   # noqa: E731
        results = {"rgb": run(geo_feats)}
        if self.dynamic_xyz_encoder is not None:
            assert dynamic_geo_feats is not None, "Dynamic geometry features are not provided."
            results["dynamic_rgb"] = run(dynamic_geo_feats)
        return results

    def query_sky(self, directions: Tensor, data_dict: Dict[str, Tensor] = None, _route: Optional[str] = None) -> Dict[str, Tensor]:
        """:660-686 (per ray).  Note: the reference does NOT remap directions for the sky head."""
        d = directions if directions.dim() == 2 else directions[:, 0]
        both = self._ray_inputs(d, data_dict)
        if both is not None:
            dd = both[1]
        else:
            dd = self.direction_encoding(d, remap=False)
            emb = self._appearance(directions, data_dict)
            if emb is not None:
                dd = torch.cat([dd, emb], dim=-1)
        if dd.dim() == 2 and (_route or self._sky_route()) == "ray_chain":
            results = {"rgb_sky": fused.skip_mlp3(dd, *skip_head_params(self.sky_head, WIDTH_CHAIN))}  # one chain launch each way (per-ray head)
        else:
            results = {"rgb_sky": self.sky_head(dd, final_act="sigmoid")}
        if self.enable_feature_head:
            results["dino_sky_feat"] = _run_sequential(self.dino_sky_head, dd)
        return results

    # ------------------------------------------------------------------ forward (:391-551)
    def forward(self, positions: Tensor, directions: Tensor = None, data_dict: Dict[str, Tensor] = {},
                return_density_only: bool = False, combine_static_dynamic: bool = False,
                query_feature_head: bool = True, query_pe_head: bool = True,
                normed_positions: Optional[Tensor] = None, hash_encodings: bool = True) -> Dict[str, Tensor]:
        """``normed_positions`` (extension): the contracted positions when the caller already has them (render_rays
        gets them from the ray-point kernel); ``positions`` may then be None unless the flow branch is on.
        ``hash_encodings`` (extension): False drops the three row-major ``*_dynamic_hash_encodings`` outputs of the flow
        branch ("to be studied" in the reference, consumed by nothing): render_rays never reads them."""
        results_dict = {}
        self._cache.clear()
        fused.clear_riders()
        if normed_positions is None:
            normed_positions = self.contract_points(positions)
        routes = self.last_routes = self._routes(positions, normed_positions, directions, data_dict, return_density_only)
        # the static colour query rides along in the neck's launch when it is the plain per-ray one (static model)
        rider = (lambda: fused.RgbRider(self._ray_inputs(directions, data_dict)[0], directions.shape[1], skip_head_params(self.rgb_head, WIDTH_64),
                                        torch.is_grad_enabled())) if routes["rgb"] == "rider" else None
        geo_feats, semantic_feats, static_density = self._split_feats(self.xyz_encoder, self.base_mlp, normed_positions, routes["static"], rider)

        dynamic = routes["dynamic"] != "none"
        if dynamic:
            normed_timestamps = timestamps_of(data_dict)
            if routes["flow"] == "batched":
                dyn = self._flow_branch(positions, normed_positions, normed_timestamps, hash_encodings, routes["warp"])
            elif routes["flow"] != "none":   # (eval-mode temporal interpolation of the flow field takes the call-by-call order)
                dyn = self._flow_call_by_call(positions, normed_positions, normed_timestamps, routes)
            else:
                dyn = _Dynamic(*self._split_feats(self.dynamic_xyz_encoder, self.dynamic_base_mlp,
                                                  self._xyzt(normed_positions, normed_timestamps), routes["dynamic"]), {})
            results_dict.update(dyn.extras)
            dynamic_geo_feats, dynamic_density = dyn.geo, dyn.density
            density = static_density + dynamic_density
            results_dict.update({"density": density, "static_density": static_density, "dynamic_density": dynamic_density})
            if return_density_only:
                return results_dict
            if directions is not None:
                rgb_results = self.query_rgb(directions, geo_feats, dynamic_geo_feats, data_dict=data_dict, _route=routes["rgb"])
                results_dict["dynamic_rgb"] = rgb_results["dynamic_rgb"]
                results_dict["static_rgb"] = rgb_results["rgb"]
                if combine_static_dynamic:
                    static_ratio = static_density / (density + 1e-6)
                    dynamic_ratio = dynamic_density / (density + 1e-6)
                    results_dict["rgb"] = static_ratio[..., None] * results_dict["static_rgb"] \
                        + dynamic_ratio[..., None] * results_dict["dynamic_rgb"]
            if self.enable_shadow_head:
                shadow_ratio = _run_sequential(self.shadow_head, dynamic_geo_feats)
                results_dict["shadow_ratio"] = shadow_ratio
                if combine_static_dynamic and "rgb" in results_dict:
                    results_dict["rgb"] = static_ratio[..., None] * results_dict["rgb"] * (1 - shadow_ratio) \
                        + dynamic_ratio[..., None] * results_dict["dynamic_rgb"]
        else:
            results_dict["density"] = static_density
            if return_density_only:
                return results_dict
            if directions is not None:
                results_dict["rgb"] = self.query_rgb(directions, geo_feats, data_dict=data_dict, _route=routes["rgb"])["rgb"]

        if self.enable_feature_head and query_feature_head:
            if self.enable_learnable_pe and query_pe_head:
                pe = F.grid_sample(self.learnable_pe_map, data_dict["pixel_coords"].reshape(1, 1, -1, 2) * 2 - 1,
                                   align_corners=False, mode="bilinear").squeeze(2).squeeze(0).permute(1, 0)
                results_dict["dino_pe"] = _run_sequential(self.pe_head, pe.contiguous())
            dino_feats = _run_sequential(self.dino_head, semantic_feats)
            if dynamic:
                dynamic_dino_feats = _run_sequential(self.dino_head, dyn.sem)
                results_dict["static_dino_feat"] = dino_feats
                results_dict["dynamic_dino_feat"] = dynamic_dino_feats
                if combine_static_dynamic:
                    static_ratio = static_density / (density + 1e-6)
                    dynamic_ratio = dynamic_density / (density + 1e-6)
                    results_dict["dino_feat"] = static_ratio[..., None] * dino_feats + dynamic_ratio[..., None] * dynamic_dino_feats
            else:
                results_dict["dino_feat"] = dino_feats

        # sky (the reference's gate looks for a key that never exists, so lidar rays skip sky only through
        # return_density_only; reproduced as is, :540-549)
        if routes["sky"] != "none":
            sky_dirs = directions[:, 0]
            reduced = {k: v[:, 0] for k, v in data_dict.items()}
            results_dict.update(self.query_sky(sky_dirs, data_dict=reduced, _route=routes["sky"]))
        return results_dict

    def query_flow(self, positions: Tensor, normed_timestamps: Tensor, query_density: bool = True) -> Dict[str, Tensor]:
        """:688-713."""
        normed_positions = self.contract_points(positions)
        flow = self.forward_flow_hash(normed_positions, normed_timestamps)
        results = {"forward_flow": flow[..., :3], "backward_flow": flow[..., 3:]}
        if query_density:
            x = self._xyzt(normed_positions, normed_timestamps)
            results["dynamic_density"] = self._split_feats(self.dynamic_xyz_encoder, self.dynamic_base_mlp, x, self._dynamic_route(False))[2]
        return results

    def query_attributes(self, positions: Tensor, normed_timestamps: Tensor = None, query_feature_head: bool = True):
        """:715-785."""
        data = {} if normed_timestamps is None else {"normed_timestamps": normed_timestamps}
        out = self.forward(positions, None, data, combine_static_dynamic=False,
                           query_feature_head=query_feature_head, query_pe_head=False)
        if "static_dino_feat" in out:
            d = out["density"].unsqueeze(-1)
            out["dino_feat"] = (out["static_density"].unsqueeze(-1) * out["static_dino_feat"]
                                + out["dynamic_density"].unsqueeze(-1) * out["dynamic_dino_feat"]) / (d + 1e-6)
        return out


class DensityField(_Boxed):
    """Proposal network: radiance_fields/radiance_field.py:788-841."""
    _box_name = "propnet aabb"

    def __init__(self, xyz_encoder: HashEncoder, aabb: Union[Tensor, List[float]] = [[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]],
                 num_dims: int = 3, density_activation: Optional[Callable] = None, unbounded: bool = False,
                 base_mlp_layer_width: int = 64) -> None:
        super().__init__(aabb, density_activation)
        self.num_dims, self.unbounded = num_dims, unbounded
        self.xyz_encoder = xyz_encoder
        self.base_mlp = nn.Sequential(nn.Linear(self.xyz_encoder.n_output_dims, base_mlp_layer_width), nn.ReLU(),
                                      nn.Linear(base_mlp_layer_width, 1))

    def density_from_normed(self, normed: Tensor) -> Tensor:
        """normed [..., 3] already contracted -> density [..., 1]."""
        enc_lm = self.xyz_encoder.tcnn_encoding.forward_level_major(normed.reshape(-1, self.num_dims))
        lin0, lin1 = self.base_mlp[0], self.base_mlp[2]
        d = fused.density_mlp(enc_lm, lin0.weight, lin0.bias, lin1.weight, lin1.bias)  # grid -> 64 -> 1 -> trunc_exp, one chain
        return d.view(*normed.shape[:-1], 1)

    def forward(self, positions: Tensor, data_dict: Dict[str, Tensor] = None) -> Dict[str, Tensor]:
        normed = ops.contract_points(positions, self.aabb.reshape(-1), self.unbounded)
        return {"density": self.density_from_normed(normed)}


def build_radiance_field_from_cfg(cfg, verbose=True) -> RadianceField:
    """radiance_fields/radiance_field.py:907-946 (including the hard-coded flow grid, :916-923)."""
    xyz_encoder = build_xyz_encoder_from_cfg(cfg.xyz_encoder, verbose=verbose)
    dynamic_xyz_encoder = flow_xyz_encoder = None
    if cfg.head.enable_dynamic_branch:
        dynamic_xyz_encoder = build_xyz_encoder_from_cfg(cfg.dynamic_xyz_encoder, verbose=verbose)
    if cfg.head.enable_flow_branch:
        flow_xyz_encoder = HashEncoder(n_input_dims=4, n_levels=10, base_resolution=16, max_resolution=4096,
                                       log2_hashmap_size=18, n_features_per_level=4, verbose=verbose)
    return RadianceField(
        xyz_encoder=xyz_encoder, dynamic_xyz_encoder=dynamic_xyz_encoder, flow_xyz_encoder=flow_xyz_encoder,
        unbounded=cfg.unbounded, num_cams=cfg.num_cams,
        geometry_feature_dim=cfg.neck.geometry_feature_dim, base_mlp_layer_width=cfg.neck.base_mlp_layer_width,
        head_mlp_layer_width=cfg.head.head_mlp_layer_width, enable_cam_embedding=cfg.head.enable_cam_embedding,
        enable_img_embedding=cfg.head.enable_img_embedding, appearance_embedding_dim=cfg.head.appearance_embedding_dim,
        enable_sky_head=cfg.head.enable_sky_head, enable_feature_head=cfg.head.enable_feature_head,
        semantic_feature_dim=cfg.neck.semantic_feature_dim, feature_mlp_layer_width=cfg.head.feature_mlp_layer_width,
        feature_embedding_dim=cfg.head.feature_embedding_dim, enable_shadow_head=cfg.head.enable_shadow_head,
        num_train_timesteps=cfg.num_train_timesteps, interpolate_xyz_encoding=cfg.head.interpolate_xyz_encoding,
        enable_learnable_pe=cfg.head.enable_learnable_pe,
        enable_temporal_interpolation=cfg.head.enable_temporal_interpolation)


def build_density_field(aabb=[[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]], type: str = "HashEncoder", n_input_dims: int = 3,
                        n_levels: int = 5, base_resolution: int = 16, max_resolution: int = 128,
                        log2_hashmap_size: int = 20, n_features_per_level: int = 2, unbounded: bool = True) -> DensityField:
    """radiance_fields/radiance_field.py:949-975."""
    if type != "HashEncoder":
        raise NotImplementedError(f"Unknown (xyz_encoder) type: {type}")
    enc = HashEncoder(n_input_dims=n_input_dims, n_levels=n_levels, base_resolution=base_resolution,
                      max_resolution=max_resolution, log2_hashmap_size=log2_hashmap_size,
                      n_features_per_level=n_features_per_level, verbose=False)
    return DensityField(xyz_encoder=enc, aabb=aabb, unbounded=unbounded)
