"""The sampler / s -> t / ray-point tests' own power, without a GPU: the numpy fp32 operation-order models of tests/_sample_probe.py
against the exact probes and random families that tests/test_sample_exact_gpu.py holds emer_importance_sample,
emer_importance_sample_points, emer_stot and emer_ray_points to.

* the un-mutated models pass every exact probe bit for bit (against the fp64 evaluation) and equal the C oracle bit for bit on
  every family (``log``: within ``LOG_ULP_CPU`` of exp of the fp32 argument); no entry of any output is excluded (cover 1.0,
  printed);
* every mutant of ``P.MUTANTS`` fails a probe of the family named for it; which probes catch it is printed.  ``P.EQUIVALENT``
  lists the one slip no input can show, and a test proves that it computes the same function;
* the six s -> t maps equal the reference's own ``_transform_stot`` as recorded in tests/golden/stot_reference.npz;
* edges are sorted and inside [v_0, v_last] on every random family.
"""
import functools
import os

import numpy as np
import pytest

from tests import _sample_probe as P

F32, F64 = np.float32, np.float64

DYADIC = [(m, n, j) for m in (2, 3, 64, 65) for n in (1, 63, 127) for j in ("default", "cycle")]
# (R, m, n, jitter): m and n on both sides of the wave width 64, one row per jitter kind at least
RANDOM = [(1, 2, 1, "none"), (3, 3, 63, "uniform"), (4, 64, 64, "edge"), (5, 65, 127, "none"), (37, 129, 128, "uniform"), (5, 300, 257, "edge"),
          (5, 9, 65, "uniform"), (4, 1537, 128, "edge"), (3, 2, 128, "edge")]
POINT_SHAPES = [(1, 1), (3, 64), (67, 128), (5, 257)]


def _fails(fn):
    try:
        with np.errstate(all="ignore"):
            fn()
    except AssertionError:
        return True
    return False


@functools.lru_cache(None)
def _sampler_builds():
    out = [P.build_dyadic(m, n, j) for m, n, j in DYADIC] + [P.build_ties(), P.build_threshold(), P.build_end_clamp()]
    return out + [P.build_random(*a) for a in RANDOM]


@functools.lru_cache(None)
def _stot_builds():
    return P.build_stot_exact() + P.build_stot_random()


@functools.lru_cache(None)
def _point_builds():
    return [f(R, S, unb) for R, S in POINT_SHAPES for unb in (True, False) for f in (P.build_points_exact, P.build_points_random)]


@functools.lru_cache(None)
def _fused_builds():
    src = [P.build_dyadic(65, 63, "cycle"), P.build_ties(), P.build_threshold(), P.build_end_clamp(), P.build_random(5, 65, 64, "uniform"),
           P.build_random(4, 129, 128, "edge"), P.build_random(3, 2, 1, "none")]
    return [P.attach_geometry(b, unb) for i, b in enumerate(src) for unb in ((True, False) if i % 2 == 0 else (True,))]


def _check_points(b, mut, label, report):
    for od in (3, 4):
        got = P.model_ray_points(b["o"], b["d"], b["ts"], b["te"], b["aabb"], b["unbounded"], b["times"] if od == 4 else None, mut)
        P.check_points(b, got, f"{label} out_dim={od}", report, od)


def _probes(family, mut, report=None):
    """[(label, thunk that raises AssertionError when the models' output (under ``mut``) fails the probe)]"""
    if family == "sampler":
        return [(b["name"], lambda b=b: P.check_sample(b, P.model_sample(b, mut), b["name"], report)) for b in _sampler_builds()]
    if family == "stot":
        return [(b["name"], lambda b=b: P.check_stot(b, P.model_stot(b["typ"], b["s"], *b["planes"], mut), b["name"], report)) for b in _stot_builds()]
    if family == "points":
        out = [(b["name"], lambda b=b: _check_points(b, mut, b["name"], report)) for b in _point_builds()]
        return out + [(f"fused {b['name']} unbounded={b['geo']['unbounded']}",
                       lambda b=b: P.check_sample_points(b, P.model_sample_points(b, mut), f"fused {b['name']} unbounded={b['geo']['unbounded']}", report))
                      for b in _fused_builds()]
    raise ValueError(family)


FAMILIES = ("sampler", "stot", "points")


# --------------------------------------------------------------------------------------------- the models pass every probe
@pytest.mark.parametrize("family", FAMILIES)
def test_models_pass_every_probe_and_the_covers_are_full(family, capsys):
    report = {}
    for label, thunk in _probes(family, "", report):
        thunk()
    with capsys.disabled():
        print(f"\n[cover] {family}: {len(report)} outputs compared on every entry, min cover {min(report.values()):.1f}")
    assert report and all(v == 1.0 for v in report.values())


def test_the_families_reach_what_they_are_for():
    builds = {b["name"]: b for b in _sampler_builds()}
    dy = [b for b in builds.values() if b["name"].startswith("dyadic")]
    assert {b["vals"].shape[1] for b in dy} == {2, 3, 64, 65} and {b["n"] + 1 for b in dy} == {2, 64, 128}
    assert any((b["st"]["u"][:, :, None] == b["cdfs"].astype(F64)[:, None, 1:-1]).any() for b in dy), "dyadic rows tie with interior CDF values too"
    ec = builds["end clamp"]
    assert F32(ec["n"]) + ec["jitter"][0] == F32(ec["n"] + 1), "the case must reach u == c_last"
    rnd = [b for b in builds.values() if b["name"].startswith("random")]
    assert {b["n"] + 1 for b in rnd} & {65, 129, 258, 66}, "n + 1 that is no power of two (the reciprocal step differs there)"
    assert any(b["jitter"] is not None and (b["jitter"] == 0).any() and (b["jitter"] == F32(1) - F32(2.0 ** -24)).any() for b in rnd)
    nan = [b for b in _point_builds() if not b["exact"] and b["R"] >= 3]
    assert nan and all(np.isnan(b["want3"]["normed"]).any() and np.isinf(b["want3"]["pos"]).any() for b in nan)


# ------------------------------------------------------------------------------------------------------------------ mutants
@pytest.mark.parametrize("name", list(P.MUTANTS))
def test_every_mutant_fails_a_probe_of_its_family(name):
    family, what = P.MUTANTS[name]
    caught = [label for label, thunk in _probes(family, name) if _fails(thunk)]
    print(f"\n[mutant] {name} ({what}): family {family}, fails {len(caught)} probes: {', '.join(caught)}")
    assert caught, f"mutant {name} passes every probe of the {family} family"


def test_mutants_are_caught_by_the_probes_made_for_them():
    """Beyond "some probe": the slips that only one construction can show are caught by that construction."""
    by = {n: {label for label, thunk in _probes(P.MUTANTS[n][0], n) if _fails(thunk)} for n in ("lower_bound", "thr_1e-9", "thr_0", "joint_clamp", "beta_default_0")}
    assert "ties" in by["lower_bound"]
    assert "threshold" in by["thr_1e-9"] and "threshold" in by["thr_0"]
    assert {"threshold", "end clamp"} <= by["joint_clamp"]
    assert any(x.startswith("dyadic") and x.endswith("default") for x in by["beta_default_0"])


def test_the_break_tested_with_le_is_the_same_function():
    """P.EQUIVALENT: at x == 0.5 both branches of either piecewise inverse give the same fp32 value, so `<=` cannot be told from
    `<`: bit for bit the same on every probe, on every fp32 value within 2^-12 of 0.5 and on NaN."""
    assert list(P.EQUIVALENT) == ["break_le"]
    half = np.array([0.5], F32).view(np.uint32)[0]
    x = np.concatenate([np.arange(half - 40_000, half + 40_000, dtype=np.uint32).view(F32), np.array([np.nan, 0.0, 1.0], F32)])
    for typ in ("uniform_lindisp", "uniform_lindisp_0"):
        a, b = P.stot_inv(typ, x), P.stot_inv(typ, x, "break_le")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not [label for label, thunk in _probes("stot", "break_le") if _fails(thunk)]


# --------------------------------------------------------------------------------------------------- the models and the oracle
def test_sampler_model_equals_the_oracle(oracle):
    n_samples = 0
    for b in _sampler_builds():
        want = oracle.importance_sample(b["vals"], b["cdfs"], b["n"], b["jitter"])
        got = P.model_sampler(b["vals"], b["cdfs"], b["n"], b["jitter"])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b["name"]
        t_min, t_max, typ = b["stot"]
        assert np.array_equal(P.model_stot(typ, got, t_min, t_max).view(np.uint32), oracle.stot(want, t_min, t_max, typ).view(np.uint32)), b["name"]
        n_samples += got.size
    assert n_samples > 10_000


def test_stot_model_equals_the_oracle(oracle, capsys):
    """Five types bit for bit; ``log``: the oracle's glibc expf against exp of the model's fp32 argument."""
    worst = 0.0
    for b in _stot_builds():
        got = oracle.stot(b["s"], b["planes"][0], b["planes"][1], b["typ"])
        if b["typ"] == "log" and not b["exact"]:
            worst = max(worst, P.check_log(b["name"], got, b["arg"], P.LOG_ULP_CPU + 0.5))
        else:
            P.check_stot(b, got, b["name"])
    with capsys.disabled():
        print(f"\n[log] glibc expf of the oracle: at most {worst:.3f} ulp from exp of the fp32 argument")


@pytest.mark.parametrize("unbounded", [True, False])
def test_points_model_equals_the_oracle_and_the_reference_expression(oracle, unbounded):
    import torch
    for b in _point_builds():
        if b["unbounded"] != unbounded:
            continue
        o, d, ts, te = (torch.from_numpy(b[k]) for k in ("o", "d", "ts", "te"))
        pos = (o[:, None, :] + d[:, None, :] * (ts + te)[..., None] / 2.0).numpy()      # render_utils.py:341
        got = P.model_ray_points(b["o"], b["d"], b["ts"], b["te"], b["aabb"], unbounded)
        P.same_bits(f"{b['name']} pos", got["pos"], pos)
        P.same_bits(f"{b['name']} normed", got["normed"], oracle.contract(pos, b["aabb"], unbounded))


# ------------------------------------------------------------------------------------------------------ the reference's own map
def test_stot_model_equals_the_recorded_reference(capsys):
    """tests/golden/stot_reference.npz (record_stot.py: the reference's _transform_stot on 320 s, three plane pairs, six types).
    Five types are bit for bit the model.  ``log``: torch's log / exp against the C library's logf and a correctly rounded exp:
    measured when recording, the largest distance is 1 ulp (as an integer distance of the bit patterns)."""
    from tests.golden import record_stot as RS
    fx = np.load(os.path.join(os.path.dirname(RS.__file__), "stot_reference.npz"))
    s = fx["s"]
    assert np.array_equal(s.view(np.uint32), RS.s_values().view(np.uint32)) and {0.0, 0.5, 1.0} <= set(s.tolist()) and s.size >= 300
    assert np.array_equal(fx["planes"], np.array(RS.PLANES)) and set(RS.TYPES) == set(P.STOT_TYPES)
    worst = {}
    for typ in RS.TYPES:
        for i, planes in enumerate(RS.PLANES):
            want, got = fx[f"t/{typ}/{i}"], P.model_stot(typ, s, *planes)
            assert want.dtype == F32
            dist = np.abs(want.view(np.int32).astype(np.int64) - got.view(np.int32).astype(np.int64))
            worst[typ] = max(worst.get(typ, 0), int(dist.max()))
            assert dist.max() <= (P.LOG_ULP_CPU if typ == "log" else 0), f"{typ} {planes}: {int((dist > 0).sum())} entries differ, by up to {int(dist.max())} ulp"
    with capsys.disabled():
        print(f"\n[stot] distance of the model from the recorded reference, in ulp: {worst}")


# --------------------------------------------------------------------------------------------------------------- invariants
def test_edges_are_sorted_and_inside_the_first_and_last_value():
    for b in _sampler_builds():
        if not b["exact"]:
            assert P.edges_sorted_and_inside(b, b["want"]["s"]), b["name"]
    for w in (8, 20):       # peakier still
        rng = np.random.default_rng(w)
        wts = (rng.random((64, 128)) ** w).astype(F32)
        c = np.concatenate([np.zeros((64, 1), F32), np.cumsum(wts, 1, dtype=F32)], 1)
        c = c / np.maximum(c[:, -1:], F32(1e-12))
        b = dict(vals=np.sort(rng.random((64, 129)).astype(F32), 1), cdfs=c)
        assert P.edges_sorted_and_inside(b, P.model_sampler(b["vals"], c, 257, rng.random(64).astype(F32)))


def test_the_build_keeps_contraction_off_in_the_sampler():
    """Bit equality with an operation-order model needs `/` and sqrtf correctly rounded and no fused multiply-add: the project's
    flags relax neither (tests/test_update_bounds_cpu.py checks the flags), and sampler.hip keeps FMA contraction off."""
    from emernerf_amd import _build
    with open(os.path.join(_build.CSRC, "sampler.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read()
