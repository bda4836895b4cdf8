"""The loss tests' own power, without a GPU: the numpy models of pixel_loss, lidar_loss, reg_losses and reduce_sum
(tests/_loss_probe.py) against the exact probes and the per-entry bounds (tests/_bounds.py pixel_bounds, lidar_bounds,
reg_partial_bound).

* the fp32 model passes every exact probe (what ``check_*_outputs`` asserts of the device too), the fp64 model equals the
  restatement;
* every mutant of ``MUTANTS`` fails a probe of the family aimed at it (named here per mutant); ``EQUIVALENT`` is empty for
  these kernels -- every listed slip changes an entry -- and anything put there is shown bitwise equal;
* on the realistic families of tests/test_loss_exact_gpu.py the bounds accept the fp32 model AND the reference's own fp32
  evaluation by torch on the CPU (F.mse_loss / binary_cross_entropy, the literal line-of-sight code, .mean()): a bound that
  refuses the reference's fp32 evaluation is wrong, not the reference.
"""
import math

import numpy as np
import pytest
import torch

from tests import _loss_probe as P
from tests._bounds import U, assert_err_bound, lidar_bounds, pixel_bounds

F32, F64 = P.F32, P.F64


def _fails(fn, *a, **k):
    try:
        with np.errstate(all="ignore"):
            fn(*a, **k)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------- reduce
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", P.REDUCE_N)
def test_reduce_model_and_mutants(n, accumulate):
    b = P.build_reduce(n)
    want = P.restate_reduce(b["x"], b["prev"], accumulate)
    assert float(P.model_reduce(b["x"], b["prev"], accumulate)) == want
    if n > 1024:
        assert float(P.model_reduce(b["x"], b["prev"], accumulate, mut="tail1024")) != want, "the probe past 1024 does not see a dropped tail"
    if accumulate:
        assert float(P.model_reduce(b["x"], b["prev"], accumulate, mut="no_accumulate")) != want


# -------------------------------------------------------------------------------------------------------------- pixel
def _pixel_model(b, dt=F32, mut="", want=("rgb", "opa")):
    return P.model_pixel(b["rgb"], b["pix"], b["opa"], b["sky"], b["w_rgb"], b["w_sky"], b["up"], b["grad_scale"], dt, mut, want)


@pytest.mark.parametrize("mode", P.PIXEL_MODES)
@pytest.mark.parametrize("R", P.PIXEL_R)
def test_pixel_model_passes_the_probes(R, mode):
    for seed in (0, 1):
        b = P.build_pixel(R, mode, seed)
        m = _pixel_model(b)
        P.check_pixel_outputs(b, m["rays"], m["total"], m["d_rgb"], m["d_opa"], f"model pixel {mode} R={R}")
        m64 = _pixel_model(b, F64)
        np.testing.assert_allclose(m64["rays"], b["ref"]["rays"], rtol=1e-14, atol=0)
        for k in ("d_rgb", "d_opa"):
            if m64[k] is not None:
                np.testing.assert_allclose(m64[k].reshape(b["ref"][k].shape), b["ref"][k], rtol=1e-14, atol=0)
        # the value does not carry grad_scale, both gradients do
        r1 = P.restate_pixel(b["rgb"], b["pix"], b["opa"], b["sky"], b["w_rgb"], b["w_sky"], b["up"], 1.0)
        assert np.array_equal(r1["rays"], b["ref"]["rays"])
        for k in ("d_rgb", "d_opa"):
            if r1[k] is not None:
                assert np.array_equal(r1[k] * b["grad_scale"], b["ref"][k])


PIXEL_AIM = {"mean3R": "rgb", "target": "sky", "noclamp": "sky", "nofloor": "sky", "gs_value": "both", "gs_dopa": "sky", "no_up": "rgb"}


@pytest.mark.parametrize("name", list(P.MUTANTS["pixel"]))
def test_every_pixel_mutant_fails_a_probe(name):
    caught = []
    for mode in P.PIXEL_MODES:
        for R in P.PIXEL_R:
            b = P.build_pixel(R, mode, 0)
            with np.errstate(all="ignore"):
                m = _pixel_model(b, mut=name)
            if _fails(P.check_pixel_outputs, b, m["rays"], m["total"], m["d_rgb"], m["d_opa"], name):
                caught.append(f"{mode} {R}")
    print(f"\n[mutant] pixel {name} ({P.MUTANTS['pixel'][name]}): fails {len(caught)} probes: {', '.join(caught)}")
    assert any(c.startswith(PIXEL_AIM[name] + " ") for c in caught), f"pixel mutant {name} is not caught by the {PIXEL_AIM[name]} family: {caught}"


# -------------------------------------------------------------------------------------------------------------- lidar
def _lidar_model(b, dt=F32, mut=""):
    return P.model_lidar(b["depth"], b["gt"], b["w"], b["t"], b["eps"], b["max_depth"], b["w_depth"], b["w_sight"], b["up"], dt, mut)


@pytest.mark.parametrize("R,S,batch", P.LIDAR_CASES)
def test_lidar_model_passes_the_probes(R, S, batch):
    seen_only_gt = False
    for seed in (0, 1, 2, 3):
        b = P.build_lidar(R, S, batch, seed)
        st = b["stats"]
        if batch == "mixed" and S >= 63 and R >= 4:
            assert st["on_lo"] >= 1 and st["on_hi"] >= 1 and st["on_gt"] >= 1 and st["near"] >= 1 and st["empty"] >= 1, st
        m = _lidar_model(b)
        what = f"model lidar {batch} R={R} S={S} seed={seed}"
        P.check_lidar_outputs(b, m["rays"], m["total"], m["d_depth"], m["d_w"], what)
        assert float(m["n_pos"]) == b["ref"]["n_pos"] and float(m["n_valid"]) == b["ref"]["n_valid"]
        m64 = _lidar_model(b, F64)
        for k in ("rays", "d_depth", "d_w"):
            np.testing.assert_allclose(m64[k], b["ref"][k], rtol=1e-12, atol=1e-15, err_msg=f"{what} {k}")   # (w - delta cancels)
        fl = P.lidar_exact_flags(b)
        if batch == "mixed" and R in (8, 16) and S >= 63:
            assert fl["d_w"][b["ref"]["empty"]].all() and fl["rays"][b["gap"]].all(), "the exact part of the probe is not exact"
            assert b["gap"].any() or seed % 2, "no ray with an emptied near band (an exact loss)"
            assert (fl["d_w"] & fl["on_gt"]).sum() >= 2, "no near-band sample on gt is held exactly"
            seen_only_gt = seen_only_gt or bool((fl["rays"] & fl["only_gt"]).any())
        if batch == "novalid":
            assert np.isfinite(m["total"]) and (m["d_depth"] == 0).all()
        if batch == "nopos":
            assert (m["d_w"] == 0).all()
    if batch == "mixed" and R in (8, 16) and S >= 63:
        assert seen_only_gt, "no ray whose only near-band sample sits on gt (a loss through norm, held exactly)"


LIDAR_AIM = {"le_empty": "mixed", "le_near_lo": "mixed", "le_near_hi": "mixed", "far": "mixed", "valid_ge": "mixed", "valid_le": "mixed",
             "clamp_strict": "allvalid", "clamp_pass": "allvalid", "mean_npos": "mixed", "mean_R": "mixed", "no_posfactor": "mixed",
             "posfactor_per_ray": "mixed", "sigma_eps": "mixed", "norm_pi": "mixed", "norm_rsqrt": "mixed", "tail_lanes": "mixed", "first64": "mixed", "skip_nonpos": "mixed"}
_MUT_SHAPES = ((1, 1), (3, 65), (4, 64), (5, 200), (8, 129), (13, 63), (16, 128))


@pytest.mark.parametrize("name", list(P.MUTANTS["lidar"]))
def test_every_lidar_mutant_fails_a_probe(name):
    caught = []
    for batch in P.LIDAR_BATCHES:
        for R, S in _MUT_SHAPES:
            b = P.build_lidar(R, S, batch, 0)
            m = _lidar_model(b, mut=name)
            if _fails(P.check_lidar_outputs, b, m["rays"], m["total"], m["d_depth"], m["d_w"], name):
                caught.append(f"{batch} {R}x{S}")
    print(f"\n[mutant] lidar {name} ({P.MUTANTS['lidar'][name]}): fails {len(caught)} probes: {', '.join(caught)}")
    assert any(c.startswith(LIDAR_AIM[name] + " ") for c in caught), f"lidar mutant {name} is not caught by the {LIDAR_AIM[name]} family: {caught}"


# ---------------------------------------------------------------------------------------------------------------- reg
def _reg_model(b, dt=F32, mut=""):
    return P.model_reg(b["T"], b["coefs"], b["base"], b["up"], b["grad_scale"], dt, mut)


@pytest.mark.parametrize("family", list(P.reg_families()))
def test_reg_model_passes_the_probes(family):
    b = P.build_reg(**P.reg_families()[family])
    m = _reg_model(b)
    P.check_reg_outputs(b, m["partials"], m["total"], m["grads"], f"model reg {family}", m["d_ff"], m["d_base"])
    m64 = _reg_model(b, F64)
    assert abs(float(m64["total"]) - b["ref"]["total"]) <= 1e-12 * abs(b["ref"]["total"])
    for k, g in m64["grads"].items():
        np.testing.assert_allclose(g, b["ref"]["grads"][k], rtol=1e-13, atol=0)
    if b["packed"]:   # the packed form is fed the same numbers as the sliced form
        s = P.build_reg(**dict(P.reg_families()[family], packed=False))
        assert s["ref"]["total"] == b["ref"]["total"]
        N = b["T"]["flow6"].shape[0]
        assert np.array_equal(b["ref"]["grads"]["flow2"][:N, 3:], s["ref"]["grads"]["fpb"]) and (b["T"]["flow2"][:N, :3] != 0).any()


REG_AIM = {"divisor": "pattern dsfc", "cycle_second": "pattern c", "swap_blocks": "packed 86", "second_half": "packed 86", "unread_nonzero": "packed 86",
           "grad_detached": "pattern c", "one_sweep": "single 1048577", "tail": "single 257", "base_scaled": "pattern d"}


@pytest.mark.parametrize("name", list(P.MUTANTS["reg"]))
def test_every_reg_mutant_fails_a_probe(name):
    caught = []
    for family, kw in P.reg_families(big=name in ("one_sweep", "tail")).items():
        b = P.build_reg(**kw)
        m = _reg_model(b, mut=name)
        if _fails(P.check_reg_outputs, b, m["partials"], m["total"], m["grads"], name, m["d_ff"], m["d_base"]):
            caught.append(family)
    print(f"\n[mutant] reg {name} ({P.MUTANTS['reg'][name]}): fails {len(caught)} probes: {', '.join(caught)}")
    assert REG_AIM[name] in caught, f"reg mutant {name} is not caught by the family {REG_AIM[name]}: {caught}"


def test_equivalent_mutants_are_bitwise_equal():
    """``EQUIVALENT`` lists the mutants that provably cannot show, with the reason; each is shown bitwise the correct model on
    every probe.  For the loss kernels the list is empty: each slip of ``MUTANTS`` fails a named probe above."""
    assert set(P.EQUIVALENT) <= {"pixel", "lidar", "reg", "reduce"}
    for family, names in P.EQUIVALENT.items():
        for name in names:
            if family == "lidar":
                for R, S in _MUT_SHAPES:
                    b = P.build_lidar(R, S, "mixed", 0)
                    m0, m1 = _lidar_model(b), _lidar_model(b, mut=name)
                    assert all(np.array_equal(m0[k], m1[k]) for k in ("rays", "d_depth", "d_w")), (name, R, S)
            elif family == "pixel":
                for R in P.PIXEL_R:
                    b = P.build_pixel(R, "both", 0)
                    m0, m1 = _pixel_model(b), _pixel_model(b, mut=name)
                    assert all(np.array_equal(m0[k], m1[k]) for k in ("rays", "d_rgb", "d_opa")), (name, R)
            else:
                for kw in P.reg_families(big=False).values():
                    b = P.build_reg(**kw)
                    m0, m1 = _reg_model(b), _reg_model(b, mut=name)
                    assert m0["total"] == m1["total"] and all(np.array_equal(m0["grads"][k], m1["grads"][k]) for k in m0["grads"]), name


# --------------------------------------------------------------------------------------------------- realistic inputs
def _sum_slack(n, abs_sum):
    """A total formed by torch's own fp32 reduction: at most ceil(log2 n) + 8 roundings on the abs-sum."""
    return (math.ceil(math.log2(max(n, 2))) + 8) * U * abs_sum


@pytest.mark.parametrize("R", [257, 513])
def test_realistic_pixel_inside_the_bounds(R):
    b = P.realistic_pixel(R)
    st, bd = b["ref"], pixel_bounds(b["ref"])
    assert (b["opa"] == 1.0).any() and (b["opa"] == np.float32(1e-6)).any(), "no mass at the clamp ends"
    m = _pixel_model(b)
    for k, ref in (("rays", "rays"), ("d_rgb", "d_rgb"), ("d_opa", "d_opa")):
        assert_err_bound(m[k], st[ref], bd[k], f"model pixel R={R} {k}")
    total, d_rgb, d_opa = P.ref_pixel_torch(b, torch.float32)
    assert_err_bound(d_rgb, st["d_rgb"], bd["d_rgb"], f"fp32 reference pixel R={R} d_rgb")
    assert_err_bound(d_opa, st["d_opa"], bd["d_opa"], f"fp32 reference pixel R={R} d_opacity")
    assert abs(total - st["total"]) <= bd["rays"].sum() + _sum_slack(3 * R, np.abs(st["rays"]).sum())
    t64, r64, o64 = P.ref_pixel_torch(b, torch.float64)
    np.testing.assert_allclose(t64, st["total"], rtol=1e-12)
    np.testing.assert_allclose(o64, st["d_opa"], rtol=1e-6)   # (torch's double floor is 1e-12, the restatement's 1e-12f)


@pytest.mark.parametrize("R,S,eps,w_sight", P.LIDAR_REAL)
def test_realistic_lidar_inside_the_bounds(R, S, eps, w_sight):
    b = P.realistic_lidar(R, S, eps, w_sight)
    st = b["ref"]
    assert st["near"].any() and st["empty"].any() and 0 < st["n_valid"] < R or R < 10
    what = f"lidar R={R} S={S} eps={eps}"
    m = _lidar_model(b)
    P.check_lidar_outputs(b, m["rays"], m["total"], m["d_depth"], m["d_w"], f"model {what}", exact=False)
    bd = lidar_bounds(st, eps)
    total, dd, dw = P.ref_lidar_torch(b, torch.float32)
    assert_err_bound(dd, st["d_depth"], bd["d_depth"], f"fp32 reference {what} d_depth")
    assert_err_bound(dw, st["d_w"], bd["d_w"], f"fp32 reference {what} d_weights")
    assert abs(total - st["total"]) <= bd["rays"].sum() + _sum_slack(R * S, np.abs(st["rays"]).sum())
    t64, dd64, dw64 = P.ref_lidar_torch(b, torch.float64)
    np.testing.assert_allclose(t64, st["total_ref"], rtol=1e-12)
    np.testing.assert_allclose(dd64, st["d_depth"], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(dw64, st["d_w"], rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize("kw", P.REG_REAL, ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_realistic_reg_inside_the_bounds(kw):
    b = P.realistic_reg(**kw)
    st = b["ref"]
    m = _reg_model(b)
    P.check_reg_realistic(b, m["partials"], m["total"], m["grads"], f"model reg {kw}")
    total, grads = P.ref_reg_torch(b, torch.float32)
    _, err = P.reg_block_refs(b)
    n = max(v.size for v in b["T"].values())
    assert abs(total - st["total"]) <= err.sum() + _sum_slack(n, sum(abs(v) for v in st["parts"].values()) + abs(b["base"]))
    P.check_reg_realistic(b, None, total, grads, f"fp32 reference reg {kw}")
    t64, g64 = P.ref_reg_torch(b, torch.float64)
    np.testing.assert_allclose(t64, st["total"], rtol=1e-12)
    for k, g in g64.items():
        np.testing.assert_allclose(g, st["grads"][k], rtol=1e-12, atol=1e-300)
