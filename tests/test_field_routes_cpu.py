"""The rules of emernerf_amd/radiance_field.py (which entry points a forward runs; the route table in its module docstring) on the host:
the shipped shapes, the shapes of tests/_field_routes.py and the edges of each rule.  They read shapes, flags and the library's host-only
queries, so no GPU is needed (as tests/test_fused_paths_cpu.py).

The drift between the three spellings of the neck rule that the code had before it was written once (``_base_split``, ``_dynamic``,
``_flow_branch_batched``) is settled here: over every grid in use and every output width they are the same predicate, and the one input
that told them apart -- a tensor that is not on the GPU -- reaches none of them, because every route starts at an encoder that refuses it."""
import types

import pytest
import torch

from tests import _field_routes as T

NS = types.SimpleNamespace
# (L, F) of every grid in use: toy static / xyzt, shipped static / xyzt, the HashEncoder defaults, the reference's flow grid
GRIDS = [(6, 4), (5, 4), (10, 4), (16, 2), (10, 4)]
HIDDEN = [64, 32, 128]


@pytest.fixture
def RF(hip_lib, monkeypatch):
    from emernerf_amd import radiance_field as M
    for k, v in T.DEFAULT_FLAGS.items():
        monkeypatch.setattr(M, k, v)
    return M


def _head(hidden=64, n_layers=3, skip=(1,), bias=True):
    """Stand-in for an MLP head: skip_head_params reads the attributes only."""
    return NS(layers=[NS(weight=object(), bias=object() if bias else None) for _ in range(n_layers)], skip_connections=list(skip),
              hidden_dims=hidden)


def _ws(dims):
    return [NS(shape=(dims[i + 1], dims[i])) for i in range(len(dims) - 1)]


def test_neck_rule_on_the_shapes_in_use(RF):
    ok = RF.neck_eligible
    assert ok(64, 64, 10, 4, 64, 128) and ok(64, 0, 10, 4, 64, 64) and ok(64, 64, 16, 2, 64, 128)   # shipped: feature, dynamic / flow, encdefaults
    assert ok(64, 0, 6, 4, 64, 64) and ok(64, 0, 5, 4, 64, 64)                                      # toy static / xyzt
    assert not ok(64, 16, 6, 4, 64, 80) and not ok(64, 16, 5, 4, 64, 80)                            # toy feature: 80 outputs
    assert not ok(64, 0, 6, 4, 32, 64)                                                              # base width 32
    assert not ok(15, 0, 10, 4, 64, 15) and not ok(15, 49, 10, 4, 64, 64)                           # the class default geometry width
    assert not ok(64, 0, 10, 4, 64, 128) and not ok(64, 64, 10, 4, 64, 64)                          # output is not [geometry | semantic]
    assert not ok(64, 0, 17, 4, 64, 64) and not ok(64, 0, 10, 3, 64, 64)                            # 68 inputs; 3 features per level


def test_neck_rule_against_the_library_and_the_three_old_spellings(RF, hip_lib):
    """emer_neck_supported accepts exactly hidden 64 and 1 / 64 / 128 outputs on these grids; with 64 geometry features and an output of
    64 + semantic width, `n_out in (64, 128)` (the extra test of the old _base_split) therefore adds nothing."""
    for L, F in GRIDS:
        for hidden in HIDDEN:
            accepted = {n for n in range(0, 260) if hip_lib.emer_neck_supported(L, F, hidden, n)}
            assert accepted == ({1, 64, 128} if hidden == 64 else set()), (L, F, hidden)
            for geo in (15, 64):
                for sem in (0, 16, 63, 64, 65, 128):
                    for n_out in (1, 63, 64, 65, 80, 128, 192, geo + sem, 64 + sem):
                        sup = bool(hip_lib.emer_neck_supported(L, F, hidden, n_out))
                        base_split = geo == 64 and n_out in (64, 128) and n_out == 64 + sem and sup     # without is_cuda
                        dynamic = batched = geo == 64 and n_out == 64 + sem and sup                      # behind is_cuda
                        assert RF.neck_eligible(geo, sem, L, F, hidden, n_out) == base_split == dynamic == batched, (L, F, hidden, geo, sem, n_out)


def test_a_cpu_tensor_reaches_no_route(RF):
    """``is_cuda`` stood in two of the three old spellings.  It chose between two routes that both start at the encoder, and the encoder
    refuses a CPU tensor either way (row-major or level-major), so the test separated nothing."""
    from emernerf_amd import _lib
    from emernerf_amd.encodings import HashEncoder
    enc = HashEncoder(n_input_dims=4, n_levels=5, base_resolution=8, max_resolution=128, log2_hashmap_size=12, n_features_per_level=4, verbose=False)
    x = torch.rand(7, 4)
    for evaluate in (enc, enc.tcnn_encoding.forward_level_major):
        with pytest.raises(_lib.EmerError):
            evaluate(x)


def test_flow_mlp_rule(RF):
    ok = RF.flow_mlp_eligible
    b = [object()] * 3
    assert ok(_ws((40, 64, 64, 6)), b, 10, 4)                                # the reference's flow grid and MLP
    assert not ok(_ws((40, 64, 64, 6)), [object(), None, object()], 10, 4)   # a Linear without bias
    assert not ok(_ws((40, 64, 6)), b[:2], 10, 4)                            # two Linears: fused.rmlp_supported would take them, the flow rule does not
    assert not ok(_ws((40, 32, 32, 6)), b, 10, 4)                            # base width 32
    assert not ok(_ws((40, 64, 64, 6)), b, 5, 4) and not ok(_ws((40, 64, 64, 6)), b, 10, 3)   # not this grid's width; 3 features per level
    assert not ok(_ws((40, 64, 64, 65)), b, 10, 4)


def test_skip_head_rule(RF):
    p, W64, WCH = RF.skip_head_params, RF.WIDTH_64, RF.WIDTH_CHAIN
    h = _head(64)
    assert p(h, W64) == p(h, WCH) == tuple(x for l in h.layers for x in (l.weight, l.bias)) and len(p(h, W64)) == 6
    assert p(_head(128), W64) is None and p(_head(128), WCH) is not None and p(_head(256), WCH) is not None
    assert p(_head(30), W64) is None and p(_head(30), WCH) is None and p(_head(68), WCH) is not None and p(_head(66), WCH) is None
    for other in (_head(64, n_layers=4), _head(64, n_layers=2), _head(64, skip=(0,)), _head(64, skip=(1, 2)), _head(64, skip=()), _head(64, bias=False), None):
        assert p(other, W64) is None and p(other, WCH) is None


def test_appearance_key_rule(RF):
    key = RF.appearance_key
    both, cam, img = {"cam_idx": 0, "img_idx": 0}, {"cam_idx": 0}, {"img_idx": 0}
    assert [key(True, False, d) for d in (both, cam, img, {})] == ["cam_idx", "cam_idx", None, None]
    assert [key(False, True, d) for d in (both, cam, img, {})] == ["img_idx", None, "img_idx", None]
    assert [key(True, True, d) for d in (both, cam, img, {})] == ["cam_idx", "cam_idx", "img_idx", None]   # cam first, then img
    assert [key(False, False, d) for d in (both, cam, img, {})] == [None] * 4


def test_time_diff_is_read_once_per_object(RF):
    m = T.build_model("dynamic", torch.device("cpu"))
    assert m.time_diff == 1 / T.T and m._time_diff_float() == 1 / T.T
    m.register_normalized_training_timesteps(torch.linspace(0, 1, T.T))      # the reference's default: a 0-dim tensor
    assert isinstance(m.time_diff, torch.Tensor) and m._time_diff_read[0] is m.time_diff   # read at the registration
    assert m._time_diff_float() == float(m.time_diff)
    m.time_diff = torch.tensor(0.25)                                           # assigned directly: read at the first use ...
    assert m._time_diff_float() == 0.25
    m.time_diff.fill_(0.5)                                                     # ... and never again for this object
    assert m._time_diff_float() == 0.25
    m.time_diff = 0.125
    assert m._time_diff_float() == 0.125


@pytest.mark.parametrize("case_id", [c for c, v in T.CASES.items() if v["routes"] is not None])
def test_routes_that_need_no_device(RF, monkeypatch, case_id):
    """The routes of the field and flow stages depend on the model, the flags, the mode and which arguments are given -- not on the
    device -- so RadianceField._routes gives them for a model on the host (the head routes need GPU tensors: tests/test_field_routes_gpu.py)."""
    c = T.CASES[case_id]
    dev = torch.device("cpu")
    with T.flags(**c.get("flags", {})):
        model = T.build_model(case_id, dev)
        pos, dirs, data, _, _ = T._inputs(case_id, dev, **c.get("inputs", {}))
        kw = c.get("kw", {})
        if c.get("call") == "query_attributes":
            dirs, data = None, {"normed_timestamps": data["normed_timestamps"]}
        got = model._routes(pos, pos, dirs, data, kw.get("return_density_only", False))
    assert set(got) == set(T.ROUTES) and all(got[k] in T.ROUTES[k] for k in got)
    for k in ("static", "dynamic", "flow", "flow_mlp", "warp", "sky"):
        assert got[k] == c["routes"][k], k
    assert (got["rgb"] == "none") == (c["routes"]["rgb"] == "none")
    assert got["ray_inputs"] == ("none" if c["routes"]["ray_inputs"] == "none" else "separate")   # no rows without the GPU, hence no rider
    assert got["rgb"] in ("none", "general" if c["routes"]["rgb"] == "general" else "per_ray")


def test_the_cases_cover_every_value_of_every_route():
    for key, values in T.ROUTES.items():
        assert {c["routes"][key] for c in T.CASES.values() if c["routes"] is not None} == values, key


def test_flow_pair_has_one_writer_and_one_reader(RF):
    from emernerf_amd import render_utils
    flow, flow2 = torch.zeros(4, 6), torch.zeros(8, 6)
    results = {k: torch.zeros(4, 3) for k in ("forward_flow", "backward_flow", "forward_pred_backward_flow", "backward_pred_forward_flow")}
    assert RF.flow_pair(results) is None and RF.flow_pair({}) is None
    RF.attach_flow_pair(results, flow, flow2)
    extras = render_utils._extras(results, *(torch.zeros(1),) * 4)
    assert all(extras[k] is results[k] for k in results)            # the tensor OBJECTS, untouched
    pair = RF.flow_pair(extras)
    assert pair[0] is flow and pair[1] is flow2
    extras["forward_pred_backward_flow"] = extras["forward_pred_backward_flow"].reshape(2, 2, 3)   # a re-made carrier loses it
    assert RF.flow_pair(extras) is None


def test_forward_cache_slots(RF):
    cache, other = RF._ForwardCache(), RF._ForwardCache()
    w, idx, d = torch.randn(4, 3, requires_grad=True), torch.tensor([0, 2, 2, 1]), torch.randn(4, 3)
    made = []
    make_rows = lambda *a: made.append(a) or object()   # noqa: E731
    emb = cache.get("embedding", RF._EmbedFn.apply, w, idx)
    assert torch.equal(emb, w[idx]) and cache.get("embedding", RF._EmbedFn.apply, w, idx) is emb      # one gather for two consumers
    rows = cache.get("ray_rows", make_rows, w, idx, d)
    assert cache.get("ray_rows", make_rows, w, idx, d) is rows and len(made) == 1
    assert cache.get("embedding", RF._EmbedFn.apply, w, idx) is emb                                    # a slot's miss leaves the other slot alone
    assert other.embedding is None and other.ray_rows is None                                          # per instance
    with torch.no_grad():
        assert cache.get("embedding", RF._EmbedFn.apply, w, idx) is not emb                            # the grad mode is part of the key
    emb = cache.get("embedding", RF._EmbedFn.apply, w, idx)
    idx[0] = 3                                                                                         # a version counter moved: never stale
    fresh = cache.get("embedding", RF._EmbedFn.apply, w, idx)
    assert fresh is not emb and torch.equal(fresh, w[idx])
    assert cache.get("embedding", RF._EmbedFn.apply, w, idx[1:]) is not fresh                          # another storage offset / shape
    cache.clear()
    assert cache.embedding is None and cache.ray_rows is None
