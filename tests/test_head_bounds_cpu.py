"""The head tests' own power, without a GPU: the numpy emulation of the bf16x3 GEMM (tests/_head_probe.py) against the exact
probes and the per-entry bound (tests/_bounds.py c_head_*).

* the probe inputs meet their preconditions: on the grid, every entry inside the 2^24-unit budget, the planes that should
  carry the value are occupied, the dropped products are zero;
* the correct emulation is bitwise the fp64 result on every probe and stays inside the derived bound on random inputs;
* every mutant (a product dropped, an l plane zeroed or read from the neighbouring k-step) fails at least one probe.
  Whether the per-entry bound catches it as well is printed: it does not (per-addition rounding count), which is why only
  the probes discriminate.
"""
import numpy as np
import pytest

from tests import _head_probe as P
from tests._bounds import U, c_head_bf16x3, c_head_fp32

SHAPES = [(64, 128, 1000), (64, 64, 777), (256, 64, 300), (16, 40, 333)]   # (outputs, K, rows): neck / hidden / dino / flow

MUTANTS = {
    "drop w_l x_h": dict(drop={("l", "h")}),
    "drop w_h x_l": dict(drop={("h", "l")}),
    "drop w_m x_m": dict(drop={("m", "m")}),
    "l plane of W zero": dict(zero_l="a"),
    "l plane of X zero": dict(zero_l="b"),
    "l plane of W from the next k-step": dict(l_next=True),
}


def _ref(a, b, c):
    return b.astype(np.float64) @ a.astype(np.float64).T + (0.0 if c is None else c.astype(np.float64))


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_probe_preconditions(kind, shape):
    n, k, m = shape
    a, b, c, qa, qb = P.probe(kind, n, k, m, seed=n + k + m)
    assert P.on_grid(a, qa) and P.on_grid(b, qb) and P.on_grid(c, qa + qb)
    units = P.abs_units(a, b, c, qa + qb)
    assert units.max() < P.BUDGET, units.max() / P.BUDGET
    ha, ma, la = P.split3(a)
    hb, mb, lb = P.split3(b)
    # the split is exact on the grid and the dropped products vanish
    assert np.array_equal(ha.astype(np.float64) + ma + la, a.astype(np.float64))
    assert np.array_equal(hb.astype(np.float64) + mb + lb, b.astype(np.float64))
    dropped = np.abs(mb) @ np.abs(la).T + np.abs(lb) @ np.abs(ma).T + np.abs(lb) @ np.abs(la).T
    assert not dropped.any(), "a dropped partial product is non-zero on the probe"
    occ_a, occ_b = P.occupancy(a), P.occupancy(b)
    if kind == "lh":
        assert occ_a["l"] >= 0.25 and occ_a["m"] >= 0.9 and occ_b == {"m": 0.0, "l": 0.0}
    elif kind == "hl":
        assert occ_b["l"] >= 0.25 and occ_b["m"] >= 0.9 and occ_a == {"m": 0.0, "l": 0.0}
    else:
        assert occ_a["m"] >= 0.4 and occ_b["m"] >= 0.4 and occ_a["l"] == 0 and occ_b["l"] == 0
    # the B-role gradients and A-role weights of the backward probes
    for role in "ab":
        x = P.operand_like(kind, 300, k, 7, role)
        assert P.on_grid(x, P.grid_q(kind, role))


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_is_exact_on_probes(kind, shape):
    n, k, m = shape
    a, b, c, qa, qb = P.probe(kind, n, k, m, seed=n + k + m)
    ref = _ref(a, b, c)
    P.assert_exact(f"bf16x3 {kind}", P.emu_gemm(a, b, c), ref)
    P.assert_exact(f"fp32 chain {kind}", P.emu_fma_chain(a, b, c), ref)
    P.assert_exact(f"bf16x3 {kind}, k-step 16", P.emu_gemm(a, b, c, ks=16), ref)   # the 32x32x16 kernels


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_mutant_fails_a_probe(name):
    n, k, m = 64, 128, 1000
    caught, bound_caught = [], []
    for kind in P.KINDS:
        a, b, c, qa, qb = P.probe(kind, n, k, m, seed=5)
        ref = _ref(a, b, c)
        got = P.emu_gemm(a, b, c, **MUTANTS[name])
        frac = float((got.astype(np.float64) != ref).mean())
        abs_sum = P.abs_units(a, b, c, 0)
        worst = float((np.abs(got - ref) / (c_head_bf16x3(k) * U * abs_sum)).max())
        caught.append((kind, frac))
        bound_caught.append(worst > 1.0)
        print(f"\n[mutant] {name}: probe {kind}: {frac:.3f} of the entries differ, worst err / bound {worst:.3f}")
    assert max(f for _, f in caught) > 0.3, f"{name} passes every probe: {caught}"
    print(f"[mutant] {name}: caught by the bound alone: {any(bound_caught)}")


@pytest.mark.parametrize("shape", SHAPES)
def test_emulation_inside_the_bound_on_random_inputs(shape):
    n, k, m = shape
    rng = np.random.default_rng(k)
    a = (rng.standard_normal((n, k)) / k ** 0.5).astype(np.float32)
    b = rng.standard_normal((m, k)).astype(np.float32)
    b[[3, m - 1], :] = 0.0              # zero rows and zero biases: those entries have abs_sum 0 and must be exactly 0
    c = (0.1 * rng.standard_normal(n)).astype(np.float32)
    c[::2] = 0.0
    ref = _ref(a, b, c)
    abs_sum = P.abs_units(a, b, c, 0)
    assert (abs_sum == 0).sum() >= 2
    for name, got, cc in (("bf16x3", P.emu_gemm(a, b, c), c_head_bf16x3(k)), ("fp32", P.emu_fma_chain(a, b, c), c_head_fp32(k))):
        err = np.abs(got - ref)
        assert (err <= cc * U * abs_sum).all(), (name, float((err / (cc * U * abs_sum)).max()))
        print(f"\n[bound] {name} k={k}: worst err / bound {float((err / (cc * U * abs_sum)).max()):.4f}")
    # the emulated mutant "drop w_l x_h" on random inputs: its error against the bound, for the record
    got = P.emu_gemm(a, b, c, drop={("l", "h")})
    print(f"[bound] drop w_l x_h on random inputs: worst err / bound {float((np.abs(got - ref) / (c_head_bf16x3(k) * U * abs_sum)).max()):.4f}")
