"""the reference's OWN Python on the four import swaps (CPU).

tests/golden/make_golden.py::run_import_swaps_case installs the swaps the way Python resolves them -- ``sys.modules`` entries for
``third_party.tcnn_modules`` -> ``emernerf_amd.tcnn_modules`` and ``nerfacc`` (+ ``nerfacc.data_specs``, ``.estimators.base``, ``.pdf``,
``.volrend``) -> ``emernerf_amd.nerfacc_compat``, exactly the names the four edited import lines (radiance_fields/encodings.py:9,
radiance_fields/render_utils.py:4-8, third_party/nerfacc_prop_net.py:11-14, loss/base.py:7) bind -- then constructs the reference's
``build_radiance_field_from_cfg`` / ``build_density_field`` unmodified and records every ``state_dict`` entry (key, shape, dtype,
sha256 of the values) and the proposal schedule in tests/golden/import_swaps.json.  Here ``emernerf_amd.radiance_field`` is
constructed from the same seeds and compared with that recording: same keys in the same order, shapes, dtypes and values.  No kernel
runs: this is the import + construction half; the binding points' arithmetic is tests/test_a_metric_shape_gpu.py.
"""
import hashlib
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "import_swaps.json")

# what the four swapped import lines take from each module
SWAPPED_NAMES = {
    "emernerf_amd.tcnn_modules": ("Encoding",),
    "emernerf_amd.nerfacc_compat": ("accumulate_along_rays", "render_transmittance_from_density", "render_weight_from_density",
                                    "RayIntervals", "AbstractEstimator", "importance_sampling", "searchsorted"),
}


def _describe(sd):
    return [[k, list(v.shape), str(v.dtype), hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()]
            for k, v in sd.items()]


def _compare(got, want, what):
    assert [e[0] for e in got] == [e[0] for e in want], (what, sorted({e[0] for e in got} ^ {e[0] for e in want}))
    for g, w in zip(got, want):
        assert g[1:3] == w[1:3], (what, g[0], "shape / dtype", g[1:3], w[1:3])
        assert g[3] == w[3], (what, g[0], "same seed, same construction order -> same initial values")


def test_reference_python_constructs_over_the_four_import_swaps(hip_lib):
    import importlib
    for mod, names in SWAPPED_NAMES.items():
        m = importlib.import_module(mod)
        missing = [n for n in names if not hasattr(m, n)]
        assert not missing, (mod, missing)
    import emernerf_amd.nerfacc_compat as NC
    import emernerf_amd.tcnn_modules as amd_tcnn
    from emernerf_amd.prop_net import PropNetEstimator, get_proposal_requires_grad_fn
    from emernerf_amd.radiance_field import build_density_field, build_radiance_field_from_cfg
    from emernerf_amd.trainer import AABB, PROP_KW, model_config
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert sorted(rec["models"]) == ["dynamic", "feature", "flow", "static"] and len(rec["props"]) == len(PROP_KW)
    for kind, want in rec["models"].items():
        torch.manual_seed(0)
        amd = build_radiance_field_from_cfg(model_config(kind, num_cams=3 if kind == "feature" else 1), verbose=False)
        enc = amd.xyz_encoder.tcnn_encoding
        assert type(enc) is amd_tcnn.Encoding and enc.params.numel() == enc.desc.n_entries * enc.desc.n_features
        _compare(_describe(amd.state_dict()), want, kind)
    for i, (kw, want) in enumerate(zip(PROP_KW, rec["props"])):
        torch.manual_seed(1)
        _compare(_describe(build_density_field(aabb=AABB, unbounded=True, **kw).state_dict()), want, f"proposal net {i}")
    est = PropNetEstimator(None, None)
    assert isinstance(est, NC.AbstractEstimator) and est.device.type == "cpu"
    sched = rec["proposal_schedule"]
    g = get_proposal_requires_grad_fn()
    assert [bool(g(s)) for s in range(*sched["steps"])] == sched["requires_grad"], "proposal schedule"
