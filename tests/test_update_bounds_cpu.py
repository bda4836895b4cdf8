"""The update-kernel tests' own power, without a GPU: the numpy fp32 operation-order models of tests/_update_probe.py against the
exact probes and the bounds that tests/test_update_exact_gpu.py holds emer_adam_step, emer_contract_bwd, emer_flow_warp_fwd / bwd
and emer_cast_f32_f16 to.

* the un-mutated models pass every exact probe bit for bit and stay inside every bound on the random families; every
  must-cover output has cover 1.0 from the reference alone (no entry is excluded; printed);
* every mutant of ``P.MUTANTS`` fails a probe of the family named for it; which probes catch it is printed;
* a plain fp32 torch evaluation on the CPU -- one step of torch.optim.Adam, autograd of the reference contraction away from
  arg-max ties -- stays inside the bounds;
* the fp32 forward model of the contraction, from which the restatements take their branch decisions, equals the oracle's
  contraction bit for bit, and the Adam probes are exact in rational arithmetic.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _update_probe as P
from tests._bounds import adam_bounds, assert_err_bound, contract_bwd_bounds

F32, F64 = np.float32, np.float64

ADAM_N = 20_011            # odd, several vectors; the GPU module runs the same builders at 100 003
# (n, off): every split of adam_kernel -- no head, head 3 / 2 / 1, a tail, head > n, head + tail only -- and the scalar kernel (None)
ADAM_SPLITS = [(ADAM_N, 0), (ADAM_N, 1), (ADAM_N + 1, 2), (ADAM_N, 3), (2, 1), (5, 2), (9, 3), (1000, None)]
CONTRACT_N = [1, 37, 4099]
CAST_N = [1, 5, 7, 8, 9, 2048 + 3]


def _fails(fn, *a, **k):
    try:
        with np.errstate(all="ignore"):
            fn(*a, **k)
    except AssertionError:
        return True
    return False


@functools.lru_cache(None)
def _adam_builds():
    out = []
    for n, off in ADAM_SPLITS:
        for var in P.ADAM_EXACT_VARIANTS:
            out.append((f"adam exact {var} n={n} off={off}", P.build_adam_exact(n, var), off))
    for i, (n, off) in enumerate(ADAM_SPLITS):
        for step in P.ADAM_STEPS:
            hp = dict(P.ADAM_HP, step=step, wd=(0.0 if (i + step) % 4 == 3 else 1e-5), gs=(1.0 if (i + step) % 3 == 2 else 1.0 / 1024))
            out.append((f"adam random n={n} off={off} step={step} wd={hp['wd']} gs={hp['gs']:.3g}", P.build_adam_random(n, hp), off))
    return out


@functools.lru_cache(None)
def _contract_builds():
    out = []
    for N in CONTRACT_N:
        for unb in (True, False):
            out.append((f"contract exact N={N} unbounded={unb}", P.build_contract_exact(N, unb)))
            out.append((f"contract random N={N} unbounded={unb}", P.build_contract_random(N, unb)))
    return out


@functools.lru_cache(None)
def _flow_builds():
    return [(f"flow {'exact' if ex else 'random'} N={N} unbounded={unb}", P.build_flow(N, unb, ex)) for N in (37, 1031) for unb in (True, False) for ex in (True, False)]


def _check_flow(b, mut, what, report=None):
    x3, x2 = P.model_flow_warp_fwd(b["pos"], b["normed"], b["ts"], b["flow"], b["noise"], b["dt"], b["aabb"], b["unbounded"], mut)
    P.check_flow_fwd(b, x3, x2, what)
    for which in P.FLOW_CONSUMERS:
        d3, d2 = P.flow_grads(b, which)
        P.check_flow_bwd(b, which, P.model_flow_warp_bwd(b["pos"], b["flow"], b["noise"], b["aabb"], b["unbounded"], d3, d2, mut), what, report)


def _check_cast(buf, start, n, mut):
    got = P.model_cast(buf, start, n, mut)
    assert (got != P.SENTINEL_F16).all(), "cast: an entry was not written"
    P.check_cast(buf[start:start + n], got, f"cast start={start} n={n}")


@functools.lru_cache(None)
def _cast_buf():
    return P.cast_sources()


def _probes(family, mut, report=None):
    """[(label, thunk that raises AssertionError when the models' output (under ``mut``) fails the probe)]"""
    if family == "adam":
        return [(label, lambda b=b, off=off, label=label: P.check_adam(b, *_pmv(b, off, mut), label, report)) for label, b, off in _adam_builds()]
    if family == "contract":
        return [(label, lambda b=b, label=label: P.check_contract_bwd(b, P.model_contract_bwd(b["pos"], b["aabb"], b["unbounded"], b["g"], mut), label, report))
                for label, b in _contract_builds()]
    if family == "flow":
        return [(label, lambda b=b, label=label: _check_flow(b, mut, label, report)) for label, b in _flow_builds()]
    if family == "cast":
        buf = _cast_buf()
        out = [(f"cast start={s} n={n}", lambda s=s, n=n: _check_cast(buf, s, n, mut)) for s in range(4) for n in CAST_N]
        return out + [("cast all sources", lambda: _check_cast(buf, 0, buf.size - 3, mut)), ("cast all sources start=1", lambda: _check_cast(buf, 1, buf.size - 3, mut))]
    raise ValueError(family)


def _pmv(b, off, mut):
    p, m, v = P.model_adam(b["p"], b["g"], b["m"], b["v"], b["hp"], off, mut)
    return p, m, v


# --------------------------------------------------------------------------------------------- the models pass every probe
@pytest.mark.parametrize("family", ["adam", "contract", "flow", "cast"])
def test_models_pass_every_probe_and_the_covers_are_full(family, capsys):
    report = {}
    for label, thunk in _probes(family, "", report):
        thunk()
    with capsys.disabled():
        if report:
            exact = {k: v for k, v in report.items() if " exact " in k}
            bound = {k: v for k, v in report.items() if " exact " not in k}
            print(f"\n[cover] {family}: {len(exact)} exact outputs, min cover {min(exact.values()):.3f}; {len(bound)} bounded outputs, every entry "
                  f"held (cover 1.000), worst model err/bound {max(bound.values()):.3f}")
    # exact outputs report their cover (share of entries compared bit for bit); bounded outputs are compared on every entry by
    # assert_err_bound, which has no exclusion: their cover is 1.0 by construction and the report holds err / bound <= 1
    assert all(v == 1.0 for k, v in report.items() if " exact " in k)
    assert all(v <= 1.0 for v in report.values())
    assert family == "cast" or report


def test_the_families_reach_what_they_are_for():
    for N in (37, 4099):
        b = P.build_contract_exact(N, True)
        st = b["st"]
        ge1 = st["ge1"]
        for k in range(3):
            for neg in (False, True):
                uk = st["u"][:, k]
                assert (ge1 & (st["k"] == k) & ((uk < 0) == neg) & (st["mag"] > 1)).any(), f"axis {k} sign {neg} is never the arg-max"
        assert (~ge1).any() and (ge1 & (st["mag"] == 1)).any() and (st["df"][ge1 & (st["mag"] == 1)] == 0).all()
        bb = P.build_contract_exact(N, False)["st"]
        assert (~bb["inside"]).any() and bb["inside"].any()
    r = P.build_contract_random(4099, True)["st"]
    assert (r["ge1"]).any() and (~r["ge1"]).any() and all((r["k"][r["ge1"]] == k).any() for k in range(3))
    b = P.build_adam_random(ADAM_N, dict(P.ADAM_HP))
    e = b["eps_block"]
    s = b["st"]["s_bc"][e]
    assert e.any() and ((s > 1e-17) & (s < 1e-13)).all(), "the eps block's sqrt(v') / bc2_sqrt is not comparable with eps"
    for x in ("g2", "v1", "m1"):       # every intermediate of the eps block stays normal
        assert (np.abs(b["st"][x][e]) > 2.0 ** -126).all()
    src = P.cast_sources()
    assert 250_000 < src.size < 270_000


def test_adam_probes_are_exact_in_rationals():
    """2000 rows of each variant, every operation of the reference in Fractions: m', v' and p' equal the fp32 values the
    builder returns, the root and both quotients are exact."""
    for var in P.ADAM_EXACT_VARIANTS:
        b = P.build_adam_exact(2000, var)
        c = {k: Fraction(P.cf(b["hp"][k])) for k in ("lr", "b1", "b2", "eps", "wd", "gs")}
        bc1, bc2 = 1 - c["b1"], 1 - c["b2"]
        assert bc2 == Fraction(1, 4)
        bc2_sqrt = Fraction(1, 2)
        pm, mm, vm = P.model_adam(b["p"], b["g"], b["m"], b["v"], b["hp"], 0)
        for i in range(2000):
            p, g, m, v = (Fraction(float(b[x][i])) for x in ("p", "g", "m", "v"))
            gi = g * c["gs"] + c["wd"] * p
            m1 = m + (gi - m) * (1 - c["b1"])
            v1 = v * c["b2"] + (1 - c["b2"]) * gi * gi
            s = Fraction(float(b["st"]["s"][i]))
            assert s * s == v1 and s >= 0
            p1 = p - c["lr"] / bc1 * (m1 / (s / bc2_sqrt + c["eps"]))
            assert (Fraction(float(mm[i])), Fraction(float(vm[i])), Fraction(float(pm[i]))) == (m1, v1, p1)


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_there_are_at_least_thirty_mutants():
    assert len(P.MUTANTS) >= 30


@pytest.mark.parametrize("name", list(P.MUTANTS))
def test_every_mutant_fails_a_probe_of_its_family(name):
    family, what = P.MUTANTS[name]
    caught = [label for label, thunk in _probes(family, name) if _fails(thunk)]
    print(f"\n[mutant] {name} ({what}): family {family}, fails {len(caught)} probes: {', '.join(caught)}")
    assert caught, f"mutant {name} passes every probe of the {family} family"


def test_eps_before_the_division_is_caught_by_the_eps_block_at_a_small_step():
    """(sqrt v' + eps) / bc2_sqrt differs from sqrt v' / bc2_sqrt + eps by eps (1 / bc2_sqrt - 1): nothing at step 25000, where
    bc2_sqrt rounds to 1; at step 1 the entries where sqrt v' is comparable with eps see it."""
    for step, must in ((1, True), (25000, False)):
        hp = dict(P.ADAM_HP, step=step)
        b = P.build_adam_random(ADAM_N, hp)
        p, m, v = P.model_adam(b["p"], b["g"], b["m"], b["v"], hp, 0, "eps_before_division")
        bad = ~(np.abs(p - b["st"]["p1"]) <= adam_bounds(b["st"])["p"])
        print(f"\n[mutant] eps_before_division step {step}: outside the bound on {bad.mean():.4f} of the entries, {bad[b['eps_block']].mean():.4f} of the eps block")
        assert bool(bad[b["eps_block"]].all()) == must and (must or not bad.any())


# ------------------------------------------------------------------------------------------- the model of the contraction
@pytest.mark.parametrize("unbounded", [True, False])
def test_contraction_model_equals_the_oracle(oracle, unbounded):
    for aabb, pos in ((P.AABB_TRAIN, P.contract_points_random(20_000, P.AABB_TRAIN, np.random.default_rng(3))),
                      (P.AABB_EXACT, P.build_contract_exact(4099, unbounded)["pos"])):
        want = oracle.contract(pos, aabb, unbounded)
        got = P.model_contract_fwd(pos, aabb, unbounded)["out"]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# --------------------------------------------------------------------------------------- the bounds accept a plain fp32 run
@pytest.mark.parametrize("step,wd,gs", [(1, 1e-5, 1.0 / 1024), (7, 0.0, 1.0), (25000, 1e-5, 1.0)])
def test_adam_bounds_accept_torch_fp32(step, wd, gs):
    """One step of torch.optim.Adam in fp32 from the same state, with hyperparameters that are exactly the c_float values and
    the gradient g gs formed in fp32.  torch groups the step like the kernel (lerp_, addcmul_, sqrt / bc2_sqrt + eps,
    addcdiv_), narrows step_size = lr / bc1 once instead of narrowing bc1 and dividing in fp32, and may fuse a
    multiply-add: no rounding beyond those the bound counts."""
    hp = dict(P.ADAM_HP, step=step, wd=wd, gs=gs)
    b = P.build_adam_random(ADAM_N, hp)
    c = b["st"]["c"]
    p = torch.nn.Parameter(torch.from_numpy(b["p"].copy()))
    opt = torch.optim.Adam([p], lr=c["lr"], eps=c["eps"], weight_decay=c["wd"], betas=(c["b1"], c["b2"]), foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(b["m"].copy()), exp_avg_sq=torch.from_numpy(b["v"].copy()))
    p.grad = torch.from_numpy(b["g"] * F32(c["gs"]))
    opt.step()
    s = opt.state[p]
    P.check_adam(b, p.detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy(), f"torch fp32 Adam step={step} wd={wd} gs={gs:.3g}")


def _torch_contract_grad(pos, aabb, unbounded, g, inside, dtype):
    p = torch.from_numpy(np.asarray(pos)).to(dtype).requires_grad_(True)
    ab = torch.from_numpy(np.asarray(aabb, F32)).to(dtype)
    lo, hi = ab[:3], ab[3:]
    v = (p - lo) / (hi - lo)
    if unbounded:
        v = v * 2 - 1
        mag = torch.linalg.norm(v, ord=float("inf"), dim=-1, keepdim=True)
        v = torch.where(mag < 1, v, (2 - 1 / mag) * (v / mag))
        v = v / 4 + 0.5
    sel = torch.from_numpy(inside[:, None]).to(dtype)
    (v * sel * torch.from_numpy(np.asarray(g)).to(dtype)).sum().backward()
    return p.grad.numpy()


@pytest.mark.parametrize("unbounded", [True, False])
def test_contract_bounds_accept_torch_autograd(unbounded):
    """The restatement IS autograd's fp64 gradient of the reference expression (to fp64 rounding) wherever the fp32 and the
    fp64 evaluation take the same branch, and autograd in fp32 stays inside the bound there as it stands: torch's fp32 graph
    groups the arg-max term differently (it differentiates (2 - 1 / mag) (v / mag) factor by factor instead of evaluating f
    and df in closed form), which costs no more than the slack the bound carries.  Rows whose mag is within 1e-6 of 1 are left
    to the models: the fp32 and the fp64 evaluation may take different branches there, and torch's amax backward splits ties."""
    b = P.build_contract_random(20_000, unbounded, seed=1)
    st = b["st"]
    ref = _torch_contract_grad(b["pos"], b["aabb"], unbounded, b["g"], st["inside"], torch.float64)
    same = np.ones(b["N"], bool) if not unbounded else (np.abs(st["mag"] - 1.0) > 1e-6) | ~st["ge1"]
    if unbounded:
        u64 = np.abs(st["u"])
        same &= (np.argmax(u64, 1) == st["k"]) | ~st["ge1"]
        same &= ~(~st["ge1"] & (u64.max(1) >= 1.0 - 1e-6))
    assert same.mean() > 0.99
    scale = np.abs(ref).max()
    assert np.abs(ref[same] - st["out"][same]).max() <= 1e-12 * scale, "the restatement is not autograd's fp64 gradient"
    got = _torch_contract_grad(b["pos"], b["aabb"], unbounded, b["g"], st["inside"], torch.float32)
    bd = contract_bwd_bounds(st)
    assert_err_bound(got[same], st["out"][same], bd[same], f"torch fp32 autograd of the contraction (unbounded={unbounded})")


def test_the_build_relaxes_neither_division_nor_sqrt():
    """The bounds count one correctly rounded operation each for `/` and sqrtf and no fused multiply-add: the project's flags
    must not relax either, and elementwise.hip must keep FMA contraction off.  (With a relaxing flag the constant of that
    operation would have to come from a sweep on the device instead.)"""
    import os
    from emernerf_amd import _build
    relaxing = ("fast-math", "-Ofast", "unsafe-math", "approx-func", "reciprocal-math", "correctly-rounded-divide-sqrt", "denormal", "flush", "fp-contract", "-ffp-model")
    assert not [f for f in _build.CXXFLAGS if any(r in f for r in relaxing)], _build.CXXFLAGS
    with open(os.path.join(_build.CSRC, "elementwise.hip")) as f:
        assert "#pragma clang fp contract(off)" in f.read()
