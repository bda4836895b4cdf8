"""Generate golden vectors by running the REFERENCE's own Python on CPU (build container only).

    python tests/golden/make_golden.py            # writes tests/golden/*.npz and import_swaps.json
    python tests/golden/make_golden.py import_swaps    # one fixture by name

/root/reference's radiance_fields / render_utils / nerfacc_prop_net are imported UNMODIFIED on top of the
import shims of oracle/ref_shims.py (CPU oracle standing in for the absent tcnn / nerfacc binaries).  Each
case records everything a second implementation needs to reproduce the run bit-for-bit in control flow:
seeded inputs, every parameter tensor (by the reference's state_dict name), the stratified jitter and
temporal-aggregation noise the reference drew, then the outputs, the loss and selected gradients.

The .npz files are committed; the GPU box has no /root/reference, so tests only ever read the fixtures.
Tables are kept tiny (log2_hashmap_size 11-13) so the fixtures stay small.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

AABB = [-20.0, -40.0, 0.0, 80.0, 40.0, 20.0]  # configs/default_config.yaml:42


def model_cfg(kind: str, tinterp: bool = False, grid: str = "toy"):
    """Nested config equivalent to configs/default_config.yaml:40-105.  ``grid``: "toy" = small tables (log2_hashmap_size 12-13) and
    narrow feature heads, so that the fixtures of the seven original cases stay small; "default" = the SHIPPED hyper-parameters of
    configs/default_config.yaml:62-105 (static xyz D3/L10/F4/16->8192/T2^20, dynamic xyzt D4/L10/F4/32->8192/T2^18, neck 64/64/64, heads
    64 wide; the flow grid is hard-coded by the reference, radiance_field.py:916-923); "encdefaults" = the same model on the
    ``HashEncoder`` class defaults (encodings.py:110-118: D3/L16/F2/16->2048/T2^19) -- the static grid BASELINE.json configs[1] names
    and bench.py times.  ``tinterp``: enable_temporal_interpolation (eval-only: the flow field between two training timesteps,
    radiance_field.py:359-389,844-905)."""
    from oracle.ref_shims import ns
    dyn = kind in ("dynamic", "flow", "feature")
    if grid == "toy":
        xyz = dict(type="HashEncoder", n_input_dims=3, n_levels=6, n_features_per_level=4, base_resolution=16,
                   max_resolution=512, log2_hashmap_size=13)
        dxyz = dict(type="HashEncoder", n_input_dims=4, n_levels=5, n_features_per_level=4,
                    base_resolution=8, max_resolution=128, log2_hashmap_size=12)
        sem, fdim, fwidth = 16, 16, 32
    else:
        assert grid in ("default", "encdefaults"), grid
        xyz = dict(type="HashEncoder", n_input_dims=3, n_levels=10, n_features_per_level=4, base_resolution=16,
                   max_resolution=8192, log2_hashmap_size=20)
        if grid == "encdefaults":
            xyz = dict(type="HashEncoder", n_input_dims=3, n_levels=16, n_features_per_level=2, base_resolution=16,
                       max_resolution=2048, log2_hashmap_size=19)
        dxyz = dict(type="HashEncoder", n_input_dims=4, n_levels=10, n_features_per_level=4,
                    base_resolution=32, max_resolution=8192, log2_hashmap_size=18)
        sem, fdim, fwidth = 64, 64, 64
    return ns(
        xyz_encoder=xyz,
        dynamic_xyz_encoder=dxyz,
        neck=dict(base_mlp_layer_width=64, geometry_feature_dim=64, semantic_feature_dim=sem),
        head=dict(head_mlp_layer_width=64, enable_cam_embedding=kind == "feature", enable_img_embedding=kind != "feature",
                  appearance_embedding_dim=16, enable_sky_head=True, enable_feature_head=kind == "feature",
                  feature_embedding_dim=fdim, feature_mlp_layer_width=fwidth, enable_learnable_pe=True,
                  enable_dynamic_branch=dyn, enable_shadow_head=dyn, interpolate_xyz_encoding=True,
                  enable_temporal_interpolation=tinterp, enable_flow_branch=kind in ("flow", "feature")),
        unbounded=True, num_cams=3 if kind == "feature" else 1, num_train_timesteps=10,
    )


def render_cfg(prop_samples, num_samples, chunk=100):
    from oracle.ref_shims import ns
    return ns(nerf=dict(sampling=dict(num_samples=num_samples),
                        propnet=dict(num_samples_per_prop=prop_samples, near_plane=0.1, far_plane=1000.0,
                                     sampling_type="uniform_lindisp")),
              render=dict(render_chunk_size=chunk))


PROP_KW = [dict(n_levels=4, max_resolution=64, log2_hashmap_size=11, n_features_per_level=1),
           dict(n_levels=4, max_resolution=128, log2_hashmap_size=12, n_features_per_level=1)]
# configs/default_config.yaml:51-58 through builders.py:99-108 (base_resolutions_per_prop is ignored by the reference: base 16)
PROP_KW_SHIPPED = [dict(n_levels=8, max_resolution=512, log2_hashmap_size=20, n_features_per_level=1),
                   dict(n_levels=8, max_resolution=2048, log2_hashmap_size=20, n_features_per_level=1)]


def prop_kw(grid: str = "toy"):
    return PROP_KW if grid == "toy" else PROP_KW_SHIPPED


def make_rays(R, seed, n_timesteps=10, num_cams=1, image_shape=None):
    """Synthetic rays of SURVEY.md section 8d."""
    g = torch.Generator().manual_seed(seed)
    o = torch.stack([torch.rand(R, generator=g) * 60, torch.rand(R, generator=g) * 4 - 2, torch.rand(R, generator=g) + 1.5], -1)
    d = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0]) + 0.6 * torch.randn(R, 3, generator=g), dim=-1)
    img_idx = torch.randint(0, n_timesteps * num_cams, (R,), generator=g)
    data = {
        "origins": o, "viewdirs": d, "direction_norms": torch.ones(R, 1),
        "pixel_coords": torch.rand(R, 2, generator=g),
        "normed_timestamps": torch.randint(0, n_timesteps, (R,), generator=g).float() / (n_timesteps - 1),
        "img_idx": img_idx, "cam_idx": img_idx % num_cams,
        "pixels": torch.rand(R, 3, generator=g), "sky_masks": (torch.rand(R, generator=g) < 0.15).float(),
        "features": torch.rand(R, 16, generator=g),
    }
    if image_shape is not None:
        H, W = image_shape
        data = {k: v.reshape(H, W, *v.shape[1:]) for k, v in data.items()}
    return data


def table_values(tag: str, numel: int, seed: int) -> torch.Tensor:
    """Deterministic U(-0.5, 0.5) table for the parameter called ``tag`` (tables are NOT stored in the
    fixtures: the reference hard-codes a 9.7 M-parameter flow grid, radiance_field.py:916-923)."""
    import zlib
    g = torch.Generator().manual_seed(seed * 1000003 + zlib.crc32(tag.encode()) % 1000003)
    return torch.rand(numel, generator=g) - 0.5


def randomize_tables(named_modules, seed):
    """tcnn's +-1e-4 init makes every output degenerate; parity runs on tables ~U(-0.5,0.5).
    named_modules: {prefix: module}; every '*tcnn_encoding.params' gets table_values(prefix + name)."""
    with torch.no_grad():
        for prefix, m in named_modules.items():
            for name, p in m.named_parameters():
                if name.endswith("tcnn_encoding.params"):
                    p.copy_(table_values(prefix + name, p.numel(), seed).to(p.device))


BIG = 200_000  # tensors above this size are stored as digests


def digest_indices(numel: int) -> torch.Tensor:
    return torch.randint(0, numel, (4096,), generator=torch.Generator().manual_seed(numel))


def put(out: dict, key: str, t: torch.Tensor):
    """Store a tensor, or for big ones a digest: 4096 sampled entries + L2 norm + sum."""
    t = t.detach().cpu()
    if t.numel() <= BIG:
        out[key] = t.numpy()
    else:
        flat = t.reshape(-1).double()
        out[key + "@sample"] = flat[digest_indices(flat.numel())].float().numpy()
        out[key + "@norm"] = flat.norm().numpy()
        out[key + "@sum"] = flat.sum().numpy()
        # the 4096 entries of largest magnitude with their positions: a gradient of a multi-million-entry table touched by a few
        # hundred samples is almost all zeros, so a uniform sample of positions says little about the entries that matter
        top = torch.topk(flat.abs(), min(4096, flat.numel())).indices.sort().values
        out[key + "@top_idx"] = top.numpy()
        out[key + "@top_val"] = flat[top].float().numpy()


def golden_loss(results, data, prefix=""):
    """The scalar every implementation back-propagates in the golden step (pieces of
    train_emernerf.py:657-741 with the default coefficients of configs/default_config.yaml:116-150)."""
    import torch.nn.functional as F
    loss = 0.0
    if "rgb" in results:
        loss = loss + F.mse_loss(results["rgb"].squeeze(), data["pixels"].squeeze())
        loss = loss + 0.001 * F.binary_cross_entropy(results["opacity"].squeeze(), 1 - data["sky_masks"].float().squeeze())
    else:  # lidar rays: depth only
        loss = loss + F.mse_loss(results["depth"].squeeze(), data["lidar_ranges"].squeeze()) * 1e-4
    ex = results["extras"]
    if "dino_feat" in results:
        loss = loss + 0.5 * F.mse_loss(results["dino_feat"], data["features"])
    if "dynamic_density" in ex:
        loss = loss + 0.01 * ex["dynamic_density"].mean()
    if "shadow_ratio" in results:
        loss = loss + 0.01 * results["shadow_ratio"].mean()
    if "forward_flow" in ex:
        cyc = 0.5 * ((ex["forward_flow"].detach() + ex["forward_pred_backward_flow"]) ** 2
                     + (ex["backward_flow"].detach() + ex["backward_pred_forward_flow"]) ** 2).mean()
        loss = loss + 0.01 * cyc
    return loss


GRAD_KEYS = ["base_mlp.0.weight", "base_mlp.2.bias", "rgb_head.layers.1.weight", "rgb_head.layers.2.weight",
             "xyz_encoder.tcnn_encoding.params", "dynamic_xyz_encoder.tcnn_encoding.params",
             "flow_xyz_encoder.tcnn_encoding.params", "dynamic_base_mlp.2.weight", "flow_mlp.4.weight",
             "shadow_head.0.weight", "appearance_embedding.weight", "sky_head.layers.0.weight", "dino_head.4.weight",
             "learnable_pe_map", "pe_head.0.weight"]


def _flat(prefix, d, out):
    for k, v in d.items():
        if isinstance(v, dict):
            _flat(prefix + k + "/", v, out)
        elif isinstance(v, torch.Tensor):
            out[prefix + k] = v.detach().cpu().numpy()


def run_case(kind: str, mode: str, R: int, prop_samples, num_samples, seed: int, image_shape=None, lidar=False, tinterp=False,
             grid: str = "toy"):
    """mode: 'train' (stratified, prop nets trained, backward) or 'eval' (decomposition, chunked).  ``tinterp``: the model is built
    with enable_temporal_interpolation and the rays carry timestamps BETWEEN the training timesteps."""
    from oracle import ref_shims
    ref_shims.install()
    import radiance_fields as ref_rf  # the reference's own package
    from radiance_fields import render_utils as ref_render
    from third_party import nerfacc_prop_net as ref_prop

    torch.manual_seed(seed)
    cfg = model_cfg(kind, tinterp, grid)
    model = ref_rf.build_radiance_field_from_cfg(cfg, verbose=False)
    model.set_aabb(AABB)
    model.register_normalized_training_timesteps(torch.linspace(0, 1, cfg.num_train_timesteps), time_diff=1 / cfg.num_train_timesteps)
    props = [ref_rf.build_density_field(aabb=AABB, unbounded=True, **kw) for kw in prop_kw(grid)]
    randomize_tables({"model/": model, **{f"prop{i}/": p for i, p in enumerate(props)}}, seed + 1)
    out_seed = seed + 1
    prop_opt = torch.optim.Adam([p for n in props for p in n.parameters()], lr=0.01, eps=1e-15, weight_decay=1e-5, betas=(0.9, 0.99))
    est = ref_prop.PropNetEstimator(prop_opt, None)
    rcfg = render_cfg(list(prop_samples), num_samples)

    data = make_rays(R, seed + 2, cfg.num_train_timesteps, cfg.num_cams, image_shape)
    if tinterp:   # off-grid timestamps (a novel-time render), a few rays exactly on a training timestep
        g = torch.Generator().manual_seed(seed + 4)
        ts = torch.rand(data["normed_timestamps"].shape, generator=g) * 0.96 + 0.02
        data["normed_timestamps"] = ts
    prefix = ""
    if lidar:
        prefix = "lidar_"
        data = {"lidar_origins": data["origins"], "lidar_viewdirs": data["viewdirs"],
                "lidar_ranges": torch.rand(R, 1, generator=torch.Generator().manual_seed(seed + 3)) * 60 + 2,
                "lidar_normed_timestamps": data["normed_timestamps"]}

    out = {}
    state = {}
    _flat("model/", dict(model.state_dict()), state)
    for i, p in enumerate(props):
        _flat(f"prop{i}/", dict(p.state_dict()), state)
    _flat("data/", data, out)
    out.update({"state/" + k: v for k, v in state.items() if not k.endswith("tcnn_encoding.params")})
    out["table_seed"] = np.array(out_seed)

    train = mode == "train"
    model.train(train); est.train(train)
    for p in props:
        p.train(train)
    ref_shims.JITTER_LOG.clear()
    noise_log = []
    orig_rand_like = torch.rand_like

    def logging_rand_like(t, *a, **k):  # temporal-aggregation noise (radiance_field.py:567-568)
        r = orig_rand_like(t, *a, **k)
        noise_log.append(r.detach().clone())
        return r

    # Smallest |pre-activation| over every Linear output of the run: a hidden unit within rounding of zero takes the other ReLU branch
    # in any second correct implementation and moves a whole row of a weight gradient by one sample's contribution (DESIGN section 8,
    # "metric-shape parity needs the product's own ReLU masks").  main() re-draws a case whose margin is below 2e-6.
    margin = [float("inf")]
    hooks = [m.register_forward_hook(lambda _m, _i, y: margin.__setitem__(0, min(margin[0], float(y.detach().abs().min()))))
             for net in [model] + props for m in net.modules() if isinstance(m, torch.nn.Linear)]
    torch.rand_like = logging_rand_like
    try:
        results = ref_render.render_rays(radiance_field=model, proposal_estimator=est, proposal_networks=props,
                                         data_dict=data, cfg=rcfg, proposal_requires_grad=train,
                                         return_decomposition=not train, prefix=prefix)
    finally:
        torch.rand_like = orig_rand_like
        for h in hooks:
            h.remove()
    out["min_abs_preactivation"] = np.array(margin[0])
    for i, j in enumerate(ref_shims.JITTER_LOG):
        out[f"jitter/{i}"] = j.numpy()
    for i, n in enumerate(noise_log):
        out[f"noise/{i}"] = n[..., 0:1].numpy()
    _flat("out/", {k: v for k, v in results.items() if k != "extras"}, out)
    _flat("extras/", results["extras"], out)

    if train:
        # proposal-network loss and its gradients (update_every_n_steps -> compute_loss, :181-238)
        prop_loss = est.compute_loss(results["extras"]["trans"], loss_scaler=1024)
        for p in props:
            p.zero_grad()
        prop_loss.backward()
        out["prop_loss"] = prop_loss.detach().numpy()
        for i, p in enumerate(props):
            # NB: render_utils.py:356-358 builds the level closures with a late-binding lambda, so every level
            # queries the LAST proposal network; the others receive no gradient (recorded as absent).
            for k, q in p.named_parameters():
                out[f"prop_has_grad/{i}/{k}"] = np.array(q.grad is not None)
                if q.grad is not None and k in ("base_mlp.0.weight", "base_mlp.2.weight", "xyz_encoder.tcnn_encoding.params"):
                    put(out, f"prop_grad/{i}/{k}", q.grad)
        loss = golden_loss(results, data, prefix)
        model.zero_grad()
        loss.backward()
        out["loss"] = loss.detach().numpy()
        named = dict(model.named_parameters())
        for k in GRAD_KEYS:
            if k in named and named[k].grad is not None:
                put(out, "grad/" + k, named[k].grad)
    return out


CASES = {
    # name: kwargs of run_case
    "static_train": dict(kind="static", mode="train", R=40, prop_samples=(32, 16), num_samples=24, seed=100),
    "dynamic_train": dict(kind="dynamic", mode="train", R=32, prop_samples=(24, 16), num_samples=16, seed=200),
    "flow_train": dict(kind="flow", mode="train", R=24, prop_samples=(24, 16), num_samples=16, seed=300),
    "flow_lidar_train": dict(kind="flow", mode="train", R=24, prop_samples=(24, 16), num_samples=16, seed=400, lidar=True),
    "feature_eval_image": dict(kind="feature", mode="eval", R=60, prop_samples=(24, 16), num_samples=16, seed=500, image_shape=(6, 10)),
    "feature_train": dict(kind="feature", mode="train", R=20, prop_samples=(16, 8), num_samples=12, seed=600),
    "static_eval_chunked": dict(kind="static", mode="eval", R=240, prop_samples=(32, 16), num_samples=24, seed=700),
}


# [r6] The same recordings at the SHIPPED grid hyper-parameters -- the level tables the benchmark and a real training run use
# (VERDICT r5 missing #3: the toy tables above never reach hashed levels of 2^18 .. 2^20 entries, 16 levels, or F = 2).  Tables are
# seeded, not stored, so the fixtures stay small (R <= 32, S = 16; gradients of the big tables as digests incl. their largest entries).
SHIPPED_CASES = {
    "static_encdefaults_train": dict(kind="static", mode="train", R=32, prop_samples=(24, 16), num_samples=16, seed=1400, grid="encdefaults"),
    "static_shipped_train": dict(kind="static", mode="train", R=32, prop_samples=(24, 16), num_samples=16, seed=1500, grid="default"),
    "dynamic_shipped_train": dict(kind="dynamic", mode="train", R=24, prop_samples=(24, 16), num_samples=16, seed=1600, grid="default"),
    "flow_shipped_train": dict(kind="flow", mode="train", R=16, prop_samples=(24, 16), num_samples=16, seed=1700, grid="default"),
}


# eval-only temporal interpolation of the flow field (its own test: the oracle restatement does not carry this option)
TINTERP_CASES = {
    "flow_eval_tinterp": dict(kind="flow", mode="eval", R=48, prop_samples=(24, 16), num_samples=16, seed=1300, tinterp=True),
}


# ---------------------------------------------------------------------------------------- N3: the evaluation render loop
def _install_video_utils_shims():
    """radiance_fields/video_utils.py imports packages that are absent here and have nothing to do with the path: imageio,
    scikit-image (SSIM), and -- through utils.visualization_tools and datasets -- matplotlib, plotly, PIL and the dataset
    readers.  They are replaced by stubs; ``render_pixels`` / ``render`` themselves run UNMODIFIED.  The stubs' only influence
    on the recorded values: ``ssim`` is 0 (SSIM is out of scope), and the flow visualiser (a colour wheel) is the identity,
    so ``forward_flows`` / ``backward_flows`` hold the rendered flow itself."""
    import importlib.util
    import types
    from oracle import ref_shims
    ref_shims.install()
    sys.modules.setdefault("imageio", types.ModuleType("imageio"))
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.metrics")
    skm.structural_similarity = lambda a, b, **k: 0.0
    sk.metrics = skm
    sys.modules["skimage"], sys.modules["skimage.metrics"] = sk, skm
    ds, dsb = types.ModuleType("datasets"), types.ModuleType("datasets.base")
    dsb.SplitWrapper = type("SplitWrapper", (), {})
    ds.base, ds.__path__ = dsb, []
    sys.modules["datasets"], sys.modules["datasets.base"] = ds, dsb
    spec = importlib.util.spec_from_file_location("datasets.metrics", os.path.join(ref_shims.REFERENCE_ROOT, "datasets", "metrics.py"))
    dm = importlib.util.module_from_spec(spec)
    sys.modules["datasets.metrics"] = dm
    spec.loader.exec_module(dm)          # the reference's own compute_psnr
    ds.metrics = dm
    import utils  # the reference's package
    vt = types.ModuleType("utils.visualization_tools")
    vt.resize_five_views = lambda imgs: imgs
    vt.to8b = lambda x: x
    vt.visualize_depth = lambda *a, **k: a[0]
    vt.scene_flow_to_rgb = lambda frame, **k: frame
    sys.modules["utils.visualization_tools"] = vt
    utils.visualization_tools = vt


class GoldenSplit:
    """What render() needs from a SplitWrapper (datasets/base/split_wrapper.py): ``split``, len, image-shaped ray dicts."""
    split = "test"

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return dict(self.images[i])


def run_render_pixels_case(kind: str, seed: int, n_images: int = 3, hw=(6, 10), prop_samples=(24, 16), num_samples=16, chunk=25):
    """radiance_fields/video_utils.py:50-468 on a stub split: every list the loop returns, plus the psnr it computes."""
    _install_video_utils_shims()
    import radiance_fields as ref_rf
    from radiance_fields import video_utils as ref_video
    from third_party import nerfacc_prop_net as ref_prop
    torch.manual_seed(seed)
    cfg = model_cfg(kind)
    model = ref_rf.build_radiance_field_from_cfg(cfg, verbose=False)
    model.set_aabb(AABB)
    if kind != "static":
        model.register_normalized_training_timesteps(torch.linspace(0, 1, cfg.num_train_timesteps), time_diff=1 / cfg.num_train_timesteps)
    props = [ref_rf.build_density_field(aabb=AABB, unbounded=True, **kw) for kw in PROP_KW]
    randomize_tables({"model/": model, **{f"prop{i}/": p for i, p in enumerate(props)}}, seed + 1)
    est = ref_prop.PropNetEstimator(None, None)
    rcfg = render_cfg(list(prop_samples), num_samples, chunk=chunk)
    H, W = hw
    images = []
    for i in range(n_images):
        d = make_rays(H * W, seed + 10 + i, cfg.num_train_timesteps, cfg.num_cams, (H, W))
        d.pop("features")
        images.append(d)
    out, state = {}, {}
    _flat("model/", dict(model.state_dict()), state)
    for i, p in enumerate(props):
        _flat(f"prop{i}/", dict(p.state_dict()), state)
    out.update({"state/" + k: v for k, v in state.items() if not k.endswith("tcnn_encoding.params")})
    out["table_seed"] = np.array(seed + 1)
    for i, d in enumerate(images):
        _flat(f"image{i}/", d, out)
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self      # render() moves every tensor with .cuda(): the build container has no GPU
    try:
        res = ref_video.render_pixels(rcfg, model, est, GoldenSplit(images), proposal_networks=props, compute_metrics=True,
                                      vis_indices=[0, 2], return_decomposition=True)
    finally:
        torch.Tensor.cuda = orig_cuda
    for k, v in res.items():
        if isinstance(v, list):
            for j, a in enumerate(v):
                out[f"res/{k}/{j}"] = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)
        else:
            out[f"scalar/{k}"] = np.asarray(float(v))
    return out


# ------------------------------------------------------------------------------ N2: ray generation / training batches
def run_pixel_source_case(seed: int = 1200, n_imgs: int = 6, hw=(12, 20), num_cams: int = 3, n_train: int = 96):
    """datasets/base/pixel_source.py UNMODIFIED (loaded by file path; stubs only for imports that have nothing to do with the
    path: omegaconf, PIL-free here, third_party.feature_extractor): ``get_rays`` (:39-76) on seeded pixels / cameras,
    ``ScenePixelSource.get_train_rays`` (:666-731; its torch.randint pixel draws are recorded with the batch) and
    ``get_render_rays`` (:733-826) on a tiny synthetic log."""
    import importlib.util
    import types
    from oracle import ref_shims
    ref_shims.install()
    fe = types.ModuleType("third_party.feature_extractor")
    fe.delete_features = fe.extract_and_save_features = lambda *a, **k: None
    sys.modules["third_party.feature_extractor"] = fe
    spec = importlib.util.spec_from_file_location("ref_pixel_source", os.path.join(ref_shims.REFERENCE_ROOT, "datasets", "base", "pixel_source.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Source(mod.ScenePixelSource):   # the abstract hooks read files; the tensors are set directly instead
        def create_all_filelist(self):
            pass

        def load_calibrations(self):
            pass

    g = torch.Generator().manual_seed(seed)
    H, W = hw
    src = Source.__new__(Source)
    src.device = torch.device("cpu")
    src._downscale_factor = src._old_downscale_factor = 1.0
    src.images = torch.rand(n_imgs, H, W, 3, generator=g)
    src.sky_masks = (torch.rand(n_imgs, H, W, generator=g) < 0.2).float()
    src.dynamic_masks, src.features = None, None
    c2w = torch.eye(4).repeat(n_imgs, 1, 1)
    for i in range(n_imgs):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g))
        c2w[i, :3, :3] = q
        c2w[i, :3, 3] = torch.randn(3, generator=g) * 10
    src.cam_to_worlds = c2w
    K = torch.tensor([[0.9 * W, 0.0, W / 2 + 0.3], [0.0, 0.8 * W, H / 2 - 0.2], [0.0, 0.0, 1.0]]).repeat(n_imgs, 1, 1)
    K[:, 0, 0] += torch.rand(n_imgs, generator=g)
    src.intrinsics = K
    src._normalized_timestamps = (torch.arange(n_imgs) // num_cams).float() / max(n_imgs // num_cams - 1, 1)
    src.cam_ids = torch.arange(n_imgs) % num_cams
    src.pixel_error_buffered = False
    # HEIGHT / WIDTH / buffer_ratio are read-only properties over data_cfg (:947-991)
    src.data_cfg = ref_shims.ns(load_size=[H, W], num_cams=num_cams, sampler=dict(buffer_ratio=0.0, buffer_downscale=4))
    out = {}
    for k in ("images", "sky_masks", "cam_to_worlds", "intrinsics", "normalized_timestamps", "cam_ids"):
        out["src/" + k] = getattr(src, k).numpy()
    # get_rays on its own: one camera per ray, pixel coordinates incl. the image corners
    n = 64
    x = torch.randint(0, W, (n,), generator=g); y = torch.randint(0, H, (n,), generator=g)
    x[:4], y[:4] = torch.tensor([0, W - 1, 0, W - 1]), torch.tensor([0, 0, H - 1, H - 1])
    cam = torch.randint(0, n_imgs, (n,), generator=g)
    o, d, nr = mod.get_rays(x, y, c2w[cam], K[cam])
    out.update({"get_rays/x": x.numpy(), "get_rays/y": y.numpy(), "get_rays/cam": cam.numpy(), "get_rays/origins": o.numpy(),
                "get_rays/viewdirs": d.numpy(), "get_rays/direction_norm": nr.numpy()})
    torch.manual_seed(seed + 1)
    batch = src.get_train_rays(n_train, candidate_indices=[0, 2, 3, 5])
    for k, v in batch.items():
        out["train/" + k] = v.numpy()
    rr = src.get_render_rays(4)
    for k, v in rr.items():
        out["render4/" + k] = v.numpy()
    return out


def run_lidar_source_case(seed: int = 1300, n_steps: int = 6, n_train: int = 80):
    """datasets/base/lidar_source.py UNMODIFIED (loaded by file path; omegaconf stubbed): ``sample_uniform_rays`` with its cached
    per-timestep subset (:223-275), ``get_train_rays`` (:277-308; its torch.randint draw is recorded with the batch) for a first
    candidate list, for a CHANGED list ("Recomputing cached indices") and for the same candidates given as a Tensor, and
    ``get_render_rays`` (:310-330), on a tiny synthetic log with scans of unequal length."""
    import importlib.util
    from oracle import ref_shims
    ref_shims.install()
    spec = importlib.util.spec_from_file_location("ref_lidar_source", os.path.join(ref_shims.REFERENCE_ROOT, "datasets", "base", "lidar_source.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Source(mod.SceneLidarSource):   # the abstract hooks read files; the tensors are set directly instead
        def create_all_filelist(self):
            pass

        def load_calibrations(self):
            pass

        def load_lidar(self):
            pass

    g = torch.Generator().manual_seed(seed)
    src = Source(ref_shims.ns(), device=torch.device("cpu"))
    counts = torch.randint(20, 60, (n_steps,), generator=g)
    steps = torch.arange(n_steps).repeat_interleave(counts)
    n = steps.numel()
    src.origins = torch.randn(n, 3, generator=g) * 5
    d = torch.randn(n, 3, generator=g)
    src.directions = d / d.norm(dim=-1, keepdim=True)
    src.ranges = torch.rand(n, 1, generator=g) * 70 + 1     # [n, 1]: torch.norm(..., keepdim=True), datasets/waymo.py:293
    src._timesteps = steps.long()
    src.register_normalized_timestamps(steps.float() / (n_steps - 1))
    out = {"src/origins": src.origins.numpy(), "src/directions": src.directions.numpy(), "src/ranges": src.ranges.numpy(),
           "src/timesteps": src._timesteps.numpy(), "src/normalized_timestamps": src.normalized_timestamps.numpy(),
           "num_timesteps": np.array(src.num_timesteps), "closest_0p37": np.array(int(src.find_closest_timestep(0.37)))}

    def record(tag, cand):
        torch.manual_seed(seed + len(tag))
        idx = src.sample_uniform_rays(n_train, candidate_indices=cand)
        torch.manual_seed(seed + len(tag))
        batch = src.get_train_rays(n_train, candidate_indices=cand)
        out[tag + "/cand"] = np.asarray(cand if not isinstance(cand, torch.Tensor) else cand.numpy())
        out[tag + "/lidar_idx"] = idx.numpy()
        out[tag + "/cached_indices"] = src.cached_indices.numpy()
        for k in ("cached_origins", "cached_directions", "cached_ranges", "cached_normalized_timestamps"):
            out[tag + "/" + k] = getattr(src, k).numpy()
        for k, v in batch.items():
            out[tag + "/batch/" + k] = v.numpy()
    record("first", [1, 3, 4])
    record("changed", [0, 2, 5, 3])              # "Recomputing cached indices"
    record("tensor", torch.tensor([0, 2, 5, 3]))   # a Tensor equal to the cache: no rebuild
    for k, v in src.get_render_rays(2).items():
        out["render2/" + k] = v.numpy()
    return out


# the reference's OWN construction code on the four import swaps, installed the way Python resolves them
# (``sys.modules`` entries for ``third_party.tcnn_modules`` -> ``emernerf_amd.tcnn_modules`` and ``nerfacc`` (+ ``.data_specs``,
# ``.estimators.base``, ``.pdf``, ``.volrend``) -> ``emernerf_amd.nerfacc_compat``).  Runs in a subprocess (the reference's top-level
# packages must not leak into this process) and prints one JSON record: per model kind and proposal net the state_dict keys, shapes,
# dtypes and a sha256 of every tensor's bytes (same seed, same construction order), and the proposal schedule.
IMPORT_SWAPS_SCRIPT = '''
import hashlib, json, sys, types
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(ref)r)
import torch
import emernerf_amd.tcnn_modules as amd_tcnn
import emernerf_amd.nerfacc_compat as NC
import third_party                                   # the reference's (empty-__init__) package
sys.modules["third_party.tcnn_modules"] = amd_tcnn   # encodings.py:9
third_party.tcnn_modules = amd_tcnn
nerfacc = types.ModuleType("nerfacc")
for name in ("accumulate_along_rays", "render_transmittance_from_density", "render_weight_from_density"):
    setattr(nerfacc, name, getattr(NC, name))        # render_utils.py:4-8, loss/base.py:7
def sub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m
sys.modules["nerfacc"] = nerfacc
nerfacc.data_specs = sub("nerfacc.data_specs", RayIntervals=NC.RayIntervals)                       # nerfacc_prop_net.py:11
nerfacc.estimators = sub("nerfacc.estimators")
nerfacc.estimators.base = sub("nerfacc.estimators.base", AbstractEstimator=NC.AbstractEstimator)   # :12
nerfacc.pdf = sub("nerfacc.pdf", importance_sampling=NC.importance_sampling, searchsorted=NC.searchsorted)   # :13
nerfacc.volrend = sub("nerfacc.volrend", render_transmittance_from_density=NC.render_transmittance_from_density)  # :14
sub("omegaconf", OmegaConf=type("OmegaConf", (), {}))   # not a swap: type annotations only on this path

from radiance_fields.radiance_field import build_radiance_field_from_cfg as ref_build, build_density_field as ref_density
from radiance_fields import render_utils as ref_render_utils
from third_party.nerfacc_prop_net import PropNetEstimator as RefEstimator, get_proposal_requires_grad_fn
import loss.base as ref_loss
import radiance_fields.encodings as ref_enc
assert ref_enc.tcnn is amd_tcnn, "encodings.py must have bound the swapped tcnn module"
assert ref_render_utils.accumulate_along_rays is NC.accumulate_along_rays and ref_loss.accumulate_along_rays is NC.accumulate_along_rays
from emernerf_amd.trainer import AABB, PROP_KW, model_config

def describe(sd):
    return [[k, list(v.shape), str(v.dtype), hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()]
            for k, v in sd.items()]

rec = {"models": {}, "props": []}
for kind in ("static", "dynamic", "flow", "feature"):
    torch.manual_seed(0)
    ref = ref_build(model_config(kind, num_cams=3 if kind == "feature" else 1), verbose=False)
    enc = ref.xyz_encoder.tcnn_encoding
    assert type(enc) is amd_tcnn.Encoding and enc.params.numel() == enc.desc.n_entries * enc.desc.n_features
    rec["models"][kind] = describe(ref.state_dict())
for kw in PROP_KW:
    torch.manual_seed(1)
    rec["props"].append(describe(ref_density(aabb=AABB, unbounded=True, **kw).state_dict()))
est = RefEstimator(None, None)
assert isinstance(est, NC.AbstractEstimator) and est.device.type == "cpu"
fn = get_proposal_requires_grad_fn()
rec["proposal_schedule"] = {"steps": [0, 3000, 7], "requires_grad": [bool(fn(s)) for s in range(0, 3000, 7)]}
print("SWAPS_RECORD " + json.dumps(rec))
'''


def run_import_swaps_case() -> dict:
    import json
    import subprocess
    from emernerf_amd import _build
    from oracle.ref_shims import REFERENCE_ROOT
    _build.build()   # tcnn_modules.Encoding builds its grid descriptor in the library
    r = subprocess.run([sys.executable, "-c", IMPORT_SWAPS_SCRIPT % {"root": ROOT, "ref": REFERENCE_ROOT}], capture_output=True,
                       text=True, timeout=600, cwd=REFERENCE_ROOT, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    line = [l for l in r.stdout.splitlines() if l.startswith("SWAPS_RECORD ")]
    assert r.returncode == 0 and len(line) == 1, r.stdout[-2000:] + "\n" + r.stderr[-4000:]
    return json.loads(line[0][len("SWAPS_RECORD "):])


RENDER_PIXELS_CASES = {
    "render_pixels_static": dict(kind="static", seed=800),
    "render_pixels_flow": dict(kind="flow", seed=900),
}


def main():
    only = sys.argv[1:]
    for name, kw in RENDER_PIXELS_CASES.items():
        if only and name not in only:
            continue
        out = run_render_pixels_case(**kw)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB; keys {sorted({k.split('/')[1] for k in out if k.startswith('res/')})}")
    if not only or "pixel_source" in only:
        out = run_pixel_source_case()
        path = os.path.join(HERE, "pixel_source.npz")
        np.savez_compressed(path, **out)
        print(f"pixel_source: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")
    if not only or "lidar_source" in only:
        out = run_lidar_source_case()
        path = os.path.join(HERE, "lidar_source.npz")
        np.savez_compressed(path, **out)
        print(f"lidar_source: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")
    if not only or "import_swaps" in only:
        import json
        rec = run_import_swaps_case()
        path = os.path.join(HERE, "import_swaps.json")
        with open(path, "w") as f:   # one tensor per line
            f.write(json.dumps(rec).replace("], [", "],\n[") + "\n")
        print(f"import_swaps: {sum(len(v) for v in rec['models'].values())} model tensors, {os.path.getsize(path) / 1e3:.0f} kB")
    for name, kw in {**CASES, **TINTERP_CASES, **SHIPPED_CASES}.items():
        if only and name not in only:
            continue
        out = run_case(**kw)
        while name in SHIPPED_CASES and float(out["min_abs_preactivation"]) < 2e-6:   # (the original cases keep their recorded seeds)
            kw = dict(kw, seed=kw["seed"] + 7)
            print(f"{name}: a pre-activation at {float(out['min_abs_preactivation']):.1e} of zero -- re-drawing with seed {kw['seed']}")
            out = run_case(**kw)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB, min |pre-activation| {float(out['min_abs_preactivation']):.2e}")


if __name__ == "__main__":
    main()
