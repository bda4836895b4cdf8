"""One case per route of the route table of emernerf_amd/radiance_field.py (its module docstring): the model, the module flags, the call
and the routes that RadianceField.forward must record in ``last_routes`` (test helper, not a test module).

The cases use only the public interface of the model and the three module flags, so the same table runs against any checkout of the
package: tests/test_field_routes_gpu.py pins the routes and the library calls of each case, tools/field_digests.py digests their results
and lists their device kernels.  emernerf_amd is imported when a case is built, never at import of this module.

Models come from tests/golden/make_golden.model_cfg plus overrides under torch.manual_seed(0), tables from make_golden.table_values.
5 rays x 8 samples (N = 40: two rays, more than one 16-row tile, a ragged last tile) unless a case says otherwise."""
import contextlib
import zlib

import torch

from tests.golden import make_golden as G

R, S = 5, 8
T = 10   # training timesteps (model_cfg)
BACKWARD = "-- backward --"   # the marker run_case puts between the two passes into a recorded list of names
DEFAULT_FLAGS = dict(FUSE_FLOW_WARP=True, BATCH_XYZT=True, FUSE_FIELD=True)
ROUTES = {   # every value of every route; the case list must cover them all
    "static": {"neck", "chain"}, "dynamic": {"none", "neck", "chain", "sequential"},
    "flow": {"none", "batched", "call_by_call", "interpolated"}, "flow_mlp": {"none", "fused", "sequential"},
    "warp": {"none", "fused", "torch"}, "rgb": {"none", "rider", "per_ray", "general"}, "sky": {"none", "ray_chain", "module"},
    "ray_inputs": {"none", "shared", "separate"},
}


def routes(static="neck", dynamic="none", flow="none", flow_mlp="none", warp="none", rgb="rider", sky="ray_chain", ray_inputs="shared"):
    return dict(static=static, dynamic=dynamic, flow=flow, flow_mlp=flow_mlp, warp=warp, rgb=rgb, sky=sky, ray_inputs=ray_inputs)


_FLOW = dict(dynamic="neck", flow="batched", flow_mlp="fused", warp="fused")
_FEATURE = dict(static="chain", dynamic="sequential", flow="call_by_call", flow_mlp="fused", rgb="per_ray")
_NO_HEADS = dict(rgb="none", sky="none", ray_inputs="none")
# id: dict(kind, [grid, tinterp], [cfg: {"section.key": value}], [flags], [mode "train" | "eval" | "eval_no_grad"], [call], [inputs:
# options of _inputs], [kw: keyword arguments of forward], routes)
CASES = {
    # (S = 16: the neck's launch takes the rider only where the samples of a ray fill whole 16-row tiles, fused.RgbRider.usable)
    "static": dict(kind="static", inputs=dict(S=16), routes=routes()),
    "static FUSE_FIELD off": dict(kind="static", inputs=dict(S=16), flags=dict(FUSE_FIELD=False), routes=routes(rgb="per_ray")),
    "static eval no_grad": dict(kind="static", inputs=dict(S=16), mode="eval_no_grad", routes=routes()),
    "dynamic": dict(kind="dynamic", routes=routes(dynamic="neck")),   # semantic width 0: the 64-wide neck; S = 8: the rider is declined
    "flow": dict(kind="flow", routes=routes(**_FLOW)),
    "flow BATCH_XYZT off": dict(kind="flow", flags=dict(BATCH_XYZT=False), routes=routes(**dict(_FLOW, flow="call_by_call", warp="none"))),
    "flow FUSE_FLOW_WARP off": dict(kind="flow", flags=dict(FUSE_FLOW_WARP=False), routes=routes(**dict(_FLOW, warp="torch"))),
    "flow hash_encodings": dict(kind="flow", kw=dict(hash_encodings=True), routes=routes(**_FLOW)),
    "flow lidar density only": dict(kind="flow", inputs=dict(lidar=True), kw=dict(return_density_only=True),
                                    routes=routes(**dict(_FLOW, **_NO_HEADS))),
    "feature": dict(kind="feature", routes=routes(**_FEATURE)),   # neck output 80: chain / sequential, the batched branch declines
    "feature default grid": dict(kind="feature", grid="default", routes=routes(**_FLOW)),   # the 128-wide neck, two-half aggregation
    "feature default grid hash_encodings": dict(kind="feature", grid="default", kw=dict(hash_encodings=True), routes=routes(**_FLOW)),
    "feature no flow": dict(kind="feature", cfg={"head.enable_flow_branch": False},
                            routes=routes(static="chain", dynamic="chain", rgb="per_ray")),
    "feature base width 32": dict(kind="feature", cfg={"neck.base_mlp_layer_width": 32},
                                  routes=routes(**dict(_FEATURE, flow_mlp="sequential"))),
    "flow eval tinterp between": dict(kind="flow", tinterp=True, mode="eval", inputs=dict(between=True),
                                      routes=routes(**dict(_FLOW, flow="interpolated", warp="none"))),
    "flow eval tinterp on steps": dict(kind="flow", tinterp=True, mode="eval",   # same routes: each evaluation's timestamps choose (data)
                                       routes=routes(**dict(_FLOW, flow="interpolated", warp="none"))),
    "static head width 128": dict(kind="static", cfg={"head.head_mlp_layer_width": 128}, routes=routes(rgb="per_ray")),
    "static head width 30": dict(kind="static", cfg={"head.head_mlp_layer_width": 30}, routes=routes(rgb="general", sky="module")),
    "static no embedding": dict(kind="static", cfg={"head.enable_img_embedding": False}, routes=routes(rgb="per_ray", ray_inputs="separate")),
    "static full directions": dict(kind="static", inputs=dict(full_dirs=True), routes=routes(rgb="general", ray_inputs="separate")),
    "static positions only": dict(kind="static", inputs=dict(normed=False), routes=routes()),
    "flow query_attributes": dict(kind="flow", call="query_attributes", routes=routes(**dict(_FLOW, **_NO_HEADS))),
    "flow query_flow": dict(kind="flow", call="query_flow", routes=None),   # no forward: the public method computes its own routes
}


@contextlib.contextmanager
def flags(**kw):
    """The three flags of emernerf_amd.radiance_field set to their defaults overridden by kw, restored on exit."""
    from emernerf_amd import radiance_field as RF
    want = dict(DEFAULT_FLAGS, **kw)
    prev = {k: getattr(RF, k) for k in want}
    for k, v in want.items():
        setattr(RF, k, v)
    try:
        yield
    finally:
        for k, v in prev.items():
            setattr(RF, k, v)


def build_model(case_id, dev):
    from emernerf_amd.radiance_field import build_radiance_field_from_cfg
    c = CASES[case_id]
    cfg = G.model_cfg(c["kind"], c.get("tinterp", False), c.get("grid", "toy"))
    for path, v in c.get("cfg", {}).items():
        section, key = path.split(".")
        setattr(getattr(cfg, section), key, v)
    torch.manual_seed(0)
    model = build_radiance_field_from_cfg(cfg, verbose=False)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if k.endswith("tcnn_encoding.params"):
                v.copy_(G.table_values("model/" + k, v.numel(), 7))
    model.set_aabb(G.AABB)
    model.to(dev)
    model.register_normalized_training_timesteps(torch.linspace(0, 1, T).to(dev), time_diff=1 / T)
    model.train(c.get("mode", "train") == "train")
    return model


def _inputs(case_id, dev, lidar=False, between=False, full_dirs=False, normed=True, S=S):
    """-> (positions, directions, data_dict, noise): seeded CPU draws; per-ray entries as the stride-0 (R, S) views render_rays passes."""
    c = CASES[case_id]
    g = torch.Generator().manual_seed(zlib.crc32(case_id.encode()) + 1)
    lo, hi = torch.tensor(G.AABB[:3]), torch.tensor(G.AABB[3:])
    pos = (lo + (hi - lo) * (torch.rand(R, S, 3, generator=g) * 1.5 - 0.25)).to(dev)   # some points outside the box: the contraction
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
    dirs = d[:, None, :].expand(R, S, 3)
    if full_dirs:   # contiguous (R, S, 3) directions that are no broadcast
        dirs = torch.nn.functional.normalize(torch.randn(R, S, 3, generator=g), dim=-1).to(dev)
    per_ray = lambda t: t.to(dev)[:, None].expand(R, S)   # noqa: E731
    data = {"cam_idx" if c["kind"] == "feature" else "img_idx": per_ray(torch.randint(0, 3 if c["kind"] == "feature" else T, (R,), generator=g))}
    if c["kind"] != "static":
        step = torch.randint(0, T - 1, (R,), generator=g).float()
        t = (step + (0.37 if between else 0.0)) / (T - 1)
        data["lidar_normed_timestamps" if lidar else "normed_timestamps"] = per_ray(t)
    if c["kind"] == "feature":
        data["pixel_coords"] = torch.rand(R, S, 2, generator=g).to(dev)
    noise = torch.rand(R, S, 1, generator=g).to(dev)
    return pos, dirs, data, noise, normed


def run_case(case_id, dev, names=None):
    """One call of the case under its flags and, where anything has a gradient, one backward seeded with CPU-drawn output gradients ->
    (model, result dictionary).  names: a list that a recorder wrapped around emernerf_amd._lib.call appends to; BACKWARD is put between
    the passes."""
    c = CASES[case_id]
    with flags(**c.get("flags", {})):
        model = build_model(case_id, dev)
        pos, dirs, data, noise, normed = _inputs(case_id, dev, **c.get("inputs", {}))
        if model.training:
            model._noise = lambda like: noise   # the temporal-aggregation noise, replayed
        call = c.get("call", "forward")
        with torch.set_grad_enabled(c.get("mode") != "eval_no_grad"):
            if call == "query_attributes":
                out = model.query_attributes(pos, data["normed_timestamps"])
            elif call == "query_flow":
                out = model.query_flow(pos, data["normed_timestamps"])
            else:
                out = model(pos, dirs, data, normed_positions=model.contract_points(pos) if normed else None,
                            **dict(dict(hash_encodings=False), **c.get("kw", {})))
        if names is not None:
            names.append(BACKWARD)
        outs = [v for _, v in sorted(out.items()) if v.requires_grad]
        if outs:
            g = torch.Generator().manual_seed(zlib.crc32(case_id.encode()))
            torch.autograd.backward(outs, [torch.randn(*o.shape, generator=g).to(dev) for o in outs])
    return model, out
