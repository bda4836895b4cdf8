"""The proposal-loss tests' own power, without a GPU: the numpy model of prop_loss_kernel (tests/_prop_probe.py) against
the exact probes and the per-entry bounds (tests/_bounds.py c_prop_*, prop_aa_bound).

* the probe inputs meet their preconditions: every intermediate up to the hinge argument is representable in fp32, each of
  the three scans has abs-sum / unit below 2^24, and every family reaches the kernel path it is built for (ties, strict
  alternation, block merge, zero-weight runs, edges on knots / outside the knots, zero-width and zero-weight proposal
  intervals); the reference's own fp32 evaluation is bitwise its fp64 evaluation there;
* the correct fp32 model is inside every bound the GPU test asserts, and exactly 0 where the hinge is inactive;
* every mutant of ``MUTANTS`` fails at least one named probe; the mutants of ``EQUIVALENT`` cannot fail on exact inputs
  (shown bitwise equal, reason next to each);
* realistic inputs: the fp32 model AND the reference's own fp32 evaluation (torch's sequential cumsum) stay inside the
  first-order bound; the tightness of the bound is printed per stage (not gated: tests/test_prop_loss_exact_gpu.py and
  DESIGN.md record the figures).
"""
import numpy as np
import pytest
import torch

from tests import _prop_probe as P
from tests._bounds import U, assert_prop_bound

SCALE = 2.0 ** -3          # a power of two: the products with scale are exact
MUT_SHAPES = ((2, 1), (31, 63), (64, 65), (100, 64), (128, 128))


def _run_model(b, scale, mut="", dt=P.F32):
    R = b["s_fin"].shape[0]
    sts = [P.model(b["s_fin"][r], b["trans"][r], b["s_p"][r], b["c_p"][r], b["pulse"], scale, dt, mut) for r in range(R)]
    return np.array([s["loss"] for s in sts]), np.stack([s["grad"] for s in sts]), sts


def _run_pdf(b, scale, mut="", dt=P.F32):
    R = b["s_fin"].shape[0]
    sts = [P.model_pdf(b["s_fin"][r], b["trans"][r], b["s_p"][r], b["c_p"][r], scale, dt, mut) for r in range(R)]
    return np.array([s["loss"] for s in sts]), np.stack([s["grad"] for s in sts]), sts


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", P.SHAPES)
@pytest.mark.parametrize("family", P.FAMILIES)
def test_probe_preconditions(family, shape, seed):
    n, m = shape
    b = P.build(4, n, m, family, seed)
    stats = [P.check_ray(r) for r in b["rays"]]
    worst = {k: max(s["units"][k] for s in stats) for k in ("slope", "pdf", "cdf")}
    print(f"\n[probe] {family} n={n} m={m} pulse=2^{int(np.log2(b['pulse']))}: scan abs-sum / unit "
          + ", ".join(f"{k} 2^{np.log2(v + 1):.1f}" for k, v in worst.items())
          + f"; ties {stats[0]['ties']}, active hinges {np.mean([s['active'] for s in stats]):.2f}")
    s0 = stats[0]
    if family == "tie" and n >= 31:
        assert all(s["ties"] >= n // 2 for s in stats), "tie probe has too few tied knots"
    if family == "alt":
        st = P.model(b["s_fin"][0], b["trans"][0], b["s_p"][0], b["c_p"][0], b["pulse"], 1.0, P.F64)
        assert s0["ties"] == 0 and np.array_equal(st["pa"], 2 * np.arange(n + 1)) and np.array_equal(st["pb"], 2 * np.arange(n + 1) + 1)
    if family == "block":
        st = P.model(b["s_fin"][0], b["trans"][0], b["s_p"][0], b["c_p"][0], b["pulse"], 1.0, P.F64)
        assert np.array_equal(st["pa"], np.arange(n + 1)) and np.array_equal(st["pb"], n + 1 + np.arange(n + 1))
    if family == "zeros" and n >= 31:
        wn = P.model(b["s_fin"][0], b["trans"][0], b["s_p"][0], b["c_p"][0], b["pulse"], 1.0, P.F64)["wn"]
        assert wn[0] == 0 and wn[-1] == 0 and wn[n // 2] == 0 and (b["trans"][0] == 0).any() and (b["trans"][0] == 1).sum() >= 2
    if family == "spike":
        assert all(s["zero_w"] == n - 1 for s in stats)
    if family == "short":
        assert all(s["outside"] == 2 for s in stats)
    if family == "onknot":
        assert all(s["on_knot"] == m + 1 for s in stats)
    if family == "zerowidth":
        assert all(s["zero_width"] >= 1 for s in stats)
    if family == "zero_wp" and m >= 40:
        assert all(s["zero_wp"] >= m // 8 for s in stats)
    if family in ("tie", "alt", "block", "short", "zero_wp") and m >= 40:
        assert 0.15 < np.mean([s["active"] for s in stats]) < 0.9
    # the reference as written is exact on the probe too: its fp32 and fp64 evaluations agree bit for bit, and with the model
    x64, pdf64, cdf64, ci64 = P.ref_stages(b["s_fin"], b["trans"], b["s_p"], b["pulse"], torch.float64)
    x32, pdf32, cdf32, ci32 = P.ref_stages(b["s_fin"], b["trans"], b["s_p"], b["pulse"], torch.float32)
    for name, a32, a64 in (("knots", x32, x64), ("pdf", pdf32, pdf64), ("cdf", cdf32, cdf64), ("CI", ci32, ci64)):
        assert np.array_equal(a32, a64), f"{family}: the reference's {name} differs between fp32 and fp64"
    _, _, sts = _run_model(b, 1.0)
    for r, st in enumerate(sts):
        assert np.array_equal(st["xr"].astype(np.float64), x64[r]) and np.array_equal(st["pdf"].astype(np.float64), pdf64[r])
        assert np.array_equal(st["cdf"].astype(np.float64), cdf64[r]) and np.array_equal(st["ci"].astype(np.float64), ci64[r])


# (the model has no workgroup structure: R = 1 / 13 at two shapes only)
@pytest.mark.parametrize("shape,R", [(s, 4) for s in P.SHAPES] + [(s, R) for s in ((31, 63), (128, 128)) for R in (1, 13)])
@pytest.mark.parametrize("family", P.FAMILIES)
def test_model_is_inside_the_probe_bounds(family, shape, R):
    n, m = shape
    ref = P.probe_reference(R, n, m, family, R % 2, SCALE)
    loss, grad, sts = _run_model(ref[0], SCALE)
    for st32, st64 in zip(sts, ref[3]):
        assert np.array_equal(st32["d"].astype(np.float64), st64["d"]), "the hinge argument is not exact in the fp32 model"
    # the fp64 model and the reference agree (the bounds take |G| from the model, the values from the reference)
    _, g64, _ = _run_model(ref[0], SCALE, dt=P.F64)
    np.testing.assert_allclose(g64, ref[2], rtol=4 * U, atol=1e-300)   # (the model holds the kernel's fp32 epsilon)
    P.check_aa_outputs(ref, SCALE, loss, grad, f"model {family} n={n} m={m} R={R}")


@pytest.mark.parametrize("name", list(P.MUTANTS))
def test_every_mutant_fails_a_probe(name):
    caught = []
    for family in P.FAMILIES:
        for n, m in MUT_SHAPES:
            ref = P.probe_reference(4, n, m, family, 0, SCALE)
            loss, grad, _ = _run_model(ref[0], SCALE, mut=name)
            try:
                P.check_aa_outputs(ref, SCALE, loss, grad, f"mutant {name}")
            except AssertionError:
                caught.append(f"{family} {n}x{m}")
    print(f"\n[mutant] {name} ({P.MUTANTS[name]}): fails {len(caught)} probes: {', '.join(caught)}")
    assert caught, f"mutant {name} passes every probe"
    # the family built for the path names it
    aimed = {"tie": "tie", "w_first": "tie", "w_last": "tie", "carry_slope": "block", "carry_pdf": "alt", "carry_cdf": "alt",
             "shift": "zero_wp", "G2": "zero_wp", "eps": "zero_wp"}[name]
    assert any(c.startswith(aimed + " ") for c in caught), f"mutant {name} is not caught by the {aimed} family: {caught}"


@pytest.mark.parametrize("name", list(P.EQUIVALENT))
def test_equivalent_mutants_cannot_fail_on_exact_inputs(name):
    """Dropped from the mutant list with the reason in _prop_probe.EQUIVALENT; shown here: bitwise the correct model."""
    for family in P.FAMILIES:
        for n, m in MUT_SHAPES:
            b = P.probe_reference(4, n, m, family, 0, SCALE)[0]
            l0, g0, _ = _run_model(b, SCALE)
            l1, g1, _ = _run_model(b, SCALE, mut=name)
            assert np.array_equal(l0, l1) and np.array_equal(g0, g1), (name, family, n, m)


# ------------------------------------------------------------------------------------------------------------ pdf mode
PDF_KINDS = ("shared", "scatter", "mixed")


@pytest.mark.parametrize("shape", P.SHAPES + ((100, 4),))
@pytest.mark.parametrize("kind", PDF_KINDS)
def test_pdf_probes_and_model(kind, shape):
    n, m = shape
    ref = P.pdf_reference(4, n, m, kind, 0, SCALE)
    stats = [P.check_pdf_ray(r) for r in ref[0]["rays"]]
    if kind == "shared" and n >= 31:
        assert all(s["shared"] >= min(n, m) // 4 for s in stats), "too few interior final edges equal to a proposal edge"
    if kind == "scatter" and n >= 31:
        assert all(s["max_hits"] >= n // 4 for s in stats), "too few final intervals scatter into one entry"
    print(f"\n[probe] pdf {kind} n={n} m={m}: shared edges {stats[0]['shared']}, max hits {stats[0]['max_hits']}, active {stats[0]['active']:.2f}")
    loss, grad, sts = _run_pdf(ref[0], SCALE)
    for st32, st64 in zip(sts, ref[3]):
        assert np.array_equal(st32["d"].astype(np.float64), st64["d"])
    _, g64, _ = _run_pdf(ref[0], SCALE, dt=P.F64)
    np.testing.assert_allclose(g64, ref[2], rtol=4 * U, atol=1e-300)   # (the model holds the kernel's fp32 epsilon)
    P.check_pdf_outputs(ref, SCALE, loss, grad, f"model pdf {kind} n={n} m={m}")


@pytest.mark.parametrize("name", list(P.MUTANTS_PDF))
def test_every_pdf_mutant_fails_a_probe(name):
    caught = []
    for kind in PDF_KINDS:
        for n, m in MUT_SHAPES + ((100, 4),):
            ref = P.pdf_reference(4, n, m, kind, 0, SCALE)
            loss, grad, _ = _run_pdf(ref[0], SCALE, mut=name)
            try:
                P.check_pdf_outputs(ref, SCALE, loss, grad, f"pdf mutant {name}")
            except AssertionError:
                caught.append(f"{kind} {n}x{m}")
    print(f"\n[mutant] pdf {name} ({P.MUTANTS_PDF[name]}): fails {len(caught)} probes: {', '.join(caught)}")
    assert caught, f"pdf mutant {name} passes every probe"
    if name == "left":
        assert any(c.startswith("shared") for c in caught)


# --------------------------------------------------------------------------------------------------- realistic inputs
REAL_SHAPES = [(13, 128, 128, 0), (13, 128, 64, 1), (5, 48, 64, 0), (5, 900, 512, 0)]


@pytest.mark.parametrize("R,n,m,level", REAL_SHAPES)
def test_realistic_inputs_inside_the_first_order_bound(oracle, R, n, m, level):
    scale = 1024.0 / (R * m)
    ref = P.realistic_reference(R, n, m, level, 7 + n + m, scale, oracle)
    b, pulse, loss64, grad64, st64, bd = ref
    assert (b["trans"] == 1.0).any() and (b["trans"] == 0.0).any(), "no empty space / no saturated tail in the inputs"
    assert all((s["d"] > 0).any() for s in st64), "a ray without an active hinge"
    what = f"R={R} n={n} m={m} pulse={pulse:.4f}"
    # the fp32 model
    loss, grad, sts = _run_model(dict(b, pulse=pulse), scale)
    for name in ("pdf", "ci"):
        t = P.tightness(np.stack([s[name] for s in sts]), np.stack([s[name] for s in st64]), np.stack([x[name] for x in bd]))
        print(f"\n[tightness] model {what} {name}: worst err / bound {t[0]:.3g}, median bound / |value| {t[1]:.3e}")
        assert_prop_bound(np.stack([s[name] for s in sts]), np.stack([s[name] for s in st64]), np.stack([x[name] for x in bd]), f"model {what} {name}")
    P.check_realistic_outputs(ref, loss, grad, f"model {what}")
    # what the bound is worth on these inputs, for the record (not gated: only the exact probes have to catch a mutant)
    if n <= 128:
        e_grad = np.stack([x["grad"] for x in bd])
        for name in P.MUTANTS:
            _, gm, _ = _run_model(dict(b, pulse=pulse), scale, mut=name)
            print(f"[mutant] {name} on realistic inputs {what}: gradient worst err / bound {P.tightness(gm, grad64, e_grad)[0]:.3g}")
    # the reference's own fp32 evaluation: sorted knots, sequential cumsum, masked max / min
    _, pdf32, _, ci32 = P.ref_stages(b["s_fin"], b["trans"], b["s_p"], pulse, torch.float32)
    _, pdf64, _, ci64 = P.ref_stages(b["s_fin"], b["trans"], b["s_p"], pulse, torch.float64)
    np.testing.assert_allclose(np.stack([s["ci"] for s in st64]), ci64, rtol=1e-9, atol=1e-12)
    assert_prop_bound(ci32, ci64, np.stack([x["ci"] for x in bd]), f"fp32 reference {what} ci")
    l32, g32 = P.ref_aa(b["s_fin"], b["trans"], b["s_p"], b["c_p"], pulse, scale, torch.float32)
    P.check_realistic_outputs(ref, l32, g32, f"fp32 reference {what}")
