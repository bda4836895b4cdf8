"""The per-ray head tests' own power, without a GPU: the numpy fp32 operation-order models of tests/_ray_probe.py against the
exact probes of tests/test_ray_exact_gpu.py and the per-entry bounds that tests/test_kernels_gpu.py adds to its three tests.

* the un-mutated models pass every probe bit for bit, and every named must-cover output has cover 1.0 from the fp64
  reference alone (printed);
* every mutant of ``P.MUTANTS`` fails a probe of the family named for it; which probes of which family catch it is printed;
* the bounds (``c_ray_pre_fwd``, ``c_ray_pre_bwd``, ``c_ray_wgrad``, ``c_embed_grad`` of tests/_bounds.py) accept a plain
  fp32 evaluation of the reference (torch matmul / index_add in fp32 on the CPU) and the models on random data.
"""
import numpy as np
import pytest
import torch

from tests import _ray_probe as P
from tests._bounds import E_SINF, assert_bound, c_embed_grad, c_ray_pre_bwd, c_ray_pre_fwd, c_ray_wgrad

F32, F64 = np.float32, np.float64


def _fails(fn, *a, **k):
    try:
        with np.errstate(all="ignore"):
            fn(*a, **k)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------ runs of the models
def _head_model(b, mut=""):
    fwd = P.model_head_fwd(b["rb_wide"], b["W1"], b["W2"], b["b2"], b["act"], mut)
    bwd = P.model_head_bwd(b["dout"], b["y"], b["a1m"], b["a2m"], b["W1"], b["W2"], b["act"], mut)
    return fwd, bwd


def _check_head(b, res, what, report=None):
    fwd, bwd = res
    P.check_head_fwd(b, *fwd, what, report)
    P.check_head_bwd(b, *bwd, what, report)


def _wgrad_check_all(jobs, mut, what, report=None):
    for i, j in enumerate(jobs):
        dw, db = P.model_wgrad(j, mut)
        P.check_wgrad(j, dw, db, f"{what} job {i}", report)


def _dirs_check(n, max_deg, remap, mut=""):
    d, grid = P.build_dirs(n)
    P.check_dir_rows(P.model_dir_rows(d, max_deg, remap, mut), d, grid, max_deg, remap, E_SINF, f"model dirs n={n} deg={max_deg} remap={remap}")


# name -> list of (probe label, thunk that raises AssertionError when the mutant is caught)
def _probes(family, mut):
    out = []
    if family == "pre":
        for Kh, H, R, null in P.PRE_SHAPES:
            b = P.build_pre(Kh, H, R, null)
            out.append((f"pre Kh={Kh} H={H} R={R}", lambda b=b: P.check_pre(b, *P.run_model_pre(b, mut), "m")))
    elif family in ("head_fwd", "head_bwd"):
        for C, act, R, nob2 in P.HEAD_CASES:
            for dense in P.HEAD_DENSE:
                b = P.build_head(C, act, R, dense, nob2)
                out.append((f"head C={C} act={act} R={R} dense={dense}", lambda b=b: _check_head(b, _head_model(b, mut), "m")))
        for R in P.CHAIN_R:
            b = P.build_chain(R)
            out.append((f"chain R={R}", lambda b=b: P.check_chain(b, *P.model_chain(b, mut), "m")))
    elif family == "wgrad":
        for M in P.WG_M:
            for pre in (0, 1):
                jobs = P.build_wgrad(M, pre)
                out.append((f"wgrad M={M} preload={pre}", lambda jobs=jobs: _wgrad_check_all(jobs, mut, "m")))
    elif family == "embed":
        for case in P.EMB_CASES:
            b = P.build_embed(*case)
            out.append((f"embed R={case[0]} n_emb={case[1]} E={case[2]} g={case[3]}", lambda b=b: P.check_embed(b, P.model_embed(b, mut), "m")))
    elif family == "dirs":
        for deg in P.DIR_DEGS:
            for remap in (False, True):
                out.append((f"dirs deg={deg} remap={remap} n=257", lambda deg=deg, remap=remap: _dirs_check(257, deg, remap, mut)))
        for R in P.CHAIN_R:
            b = P.build_chain(R)
            out.append((f"chain R={R}", lambda b=b: P.check_chain(b, *P.model_chain(b, mut), "m")))
    else:
        raise ValueError(family)
    return out


# ----------------------------------------------------------------------------------------------- the models pass the probes
@pytest.mark.parametrize("family", ["pre", "head_fwd", "wgrad", "embed", "dirs"])
def test_models_pass_every_probe_and_the_covers_are_full(family, capsys):
    for label, thunk in _probes(family, ""):
        thunk()
    # the covers, from the fp64 reference alone
    report = {}
    if family == "pre":
        for Kh, H, R, null in P.PRE_SHAPES:
            b = P.build_pre(Kh, H, R, null)
            assert (b["u_rb"] < P.BUDGET).all() and (b["u_dh"] < P.BUDGET).all()
            P.check_pre(b, *P.run_model_pre(b), f"Kh={Kh} H={H} R={R}", report)
    elif family == "head_fwd":
        for C, act, R, nob2 in P.HEAD_CASES:
            for dense in P.HEAD_DENSE:
                b = P.build_head(C, act, R, dense, nob2)
                f, w = b["fwd"], b["bwd"]
                assert (f["u_a2"] < P.BUDGET).all() and (w["u_d1"] < P.BUDGET).all() and (w["u_d0"] < P.BUDGET).all()
                assert dense == 1 or (f["u_out"] < P.BUDGET).all()
                # the probe reaches what it is for: live and dead units in both layers, zeros of both signs in the masks
                assert R < 8 or ((f["a2"] > 0).any() and (f["a2"] == 0).any() and (w["dpre0"] != 0).any())
                _check_head(b, _head_model(b), f"C={C} act={act} R={R} dense={dense}", report)
    elif family == "wgrad":
        for M in P.WG_M:
            for pre in (0, 1):
                jobs = P.build_wgrad(M, pre)
                for j in jobs:
                    assert (j["u_dw"] < P.BUDGET).all() and (not j["bias"] or (j["u_db"] < P.BUDGET).all())
                _wgrad_check_all(jobs, "", f"M={M} preload={pre}", report)
    elif family == "embed":
        for case in P.EMB_CASES:
            b = P.build_embed(*case)
            assert (b["u_dw"] < P.BUDGET).all()
            P.check_embed(b, P.model_embed(b), f"R={case[0]} n_emb={case[1]} E={case[2]}", report)
        b = P.build_embed(8192, 1, 16, "ab")
        assert (b["idx_wide"][:, 1] == 0).all(), "the full-list case must send every ray to row 0 (512 entries per wave)"
    with capsys.disabled():
        if report:
            print(f"\n[cover] {family}: {len(report)} outputs, min cover {min(report.values()):.3f}")
    must = {k: v for k, v in report.items() if not k.endswith(" out")}
    assert all(v == 1.0 for v in must.values()), {k: v for k, v in must.items() if v != 1.0}


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_there_are_at_least_twenty_mutants():
    assert len(P.MUTANTS) >= 20


@pytest.mark.parametrize("name", list(P.MUTANTS))
def test_every_mutant_fails_a_probe_of_its_family(name):
    family, what = P.MUTANTS[name]
    caught = [label for label, thunk in _probes(family, name) if _fails(thunk)]
    print(f"\n[mutant] {name} ({what}): family {family}, fails {len(caught)} probes: {', '.join(caught)}")
    assert caught, f"mutant {name} passes every probe of the {family} family"


# ------------------------------------------------------------------------------------- the bounds accept a plain fp32 run
@pytest.mark.parametrize("R,Kh,H", [(45, 33, 64), (70, 7, 16), (257, 64, 64)])
def test_pre_bounds_accept_fp32(R, Kh, H):
    g = torch.Generator().manual_seed(R + Kh)
    wa, wb, ba, bb, h = (torch.randn(*s, generator=g) for s in ((H, Kh), (H, Kh), (H,), (H,), (R, Kh)))
    s0, s1 = torch.randn(R, H, generator=g), torch.randn(R, H, generator=g)
    ref = torch.cat([h.double() @ wa.double().T + ba.double(), h.double() @ wb.double().T + bb.double()], 1).numpy()
    mag = torch.cat([h.abs().double() @ wa.abs().double().T + ba.abs().double(), h.abs().double() @ wb.abs().double().T + bb.abs().double()], 1).numpy()
    plain = torch.cat([h @ wa.T + ba, h @ wb.T + bb], 1).numpy()
    model = P.model_pre_fwd(h.numpy(), wa.numpy(), ba.numpy(), wb.numpy(), bb.numpy())
    for name, got in (("torch fp32", plain), ("model", model)):
        assert_bound(got, ref, mag, c_ray_pre_fwd(Kh), f"ray_pre_fwd {name} R={R} Kh={Kh} H={H}")
    ref = (s0.double() @ wa.double() + s1.double() @ wb.double()).numpy()
    mag = (s0.abs().double() @ wa.abs().double() + s1.abs().double() @ wb.abs().double()).numpy()
    for name, got in (("torch fp32", (s0 @ wa + s1 @ wb).numpy()), ("model", P.model_pre_bwd(s0.numpy(), s1.numpy(), wa.numpy(), wb.numpy()))):
        assert_bound(got, ref, mag, c_ray_pre_bwd(H), f"ray_pre_bwd {name} R={R} Kh={Kh} H={H}")


@pytest.mark.parametrize("M", [1, 300, 1000])
def test_wgrad_bound_accepts_fp32(M):
    g = torch.Generator().manual_seed(M)
    n, w = 64, 49
    dy, x = torch.randn(M + 1, n + 2, generator=g), torch.randn(M + 1, w + 3, generator=g)
    j = dict(M=M, n=n, widths=(w,), bias=True, dy_wide=dy.numpy(), x_wide=[x.numpy()], dst=[0], dw0=np.ones((n, w), F32), db0=np.ones(n, F32))
    dw, db = P.model_wgrad(j)
    d, xx = dy[:M, :n], x[:M, :w]
    ref, mag = 1.0 + (d.double().T @ xx.double()).numpy(), 1.0 + (d.abs().double().T @ xx.abs().double()).numpy()
    for name, got in (("torch fp32", (1.0 + d.T @ xx).numpy()), ("model", dw)):
        assert_bound(got, ref, mag, c_ray_wgrad(M), f"ray_wgrad dW {name} M={M}")
    assert_bound(db, 1.0 + d.double().sum(0).numpy(), 1.0 + d.abs().double().sum(0).numpy(), c_ray_wgrad(M), f"ray_wgrad db model M={M}")


@pytest.mark.parametrize("R,n_emb,E", [(37, 3, 16), (8192, 2, 16), (9000, 1, 20)])
def test_embed_bound_accepts_fp32(R, n_emb, E):
    rng = np.random.default_rng(R)
    b = dict(R=R, n_emb=n_emb, E=E, idx_wide=np.stack([np.zeros(R, np.int64), rng.integers(0, n_emb, R)], 1),
             ga_wide=rng.standard_normal((R, P.EMB_P + E)).astype(F32), gb_wide=rng.standard_normal((R, P.EMB_P + E)).astype(F32),
             dw0=np.zeros((n_emb, E), F32))
    idx = torch.from_numpy(b["idx_wide"][:, 1])
    ga, gb = torch.from_numpy(b["ga_wide"][:, P.EMB_P:]), torch.from_numpy(b["gb_wide"][:, P.EMB_P:])
    ref = torch.zeros(n_emb, E, dtype=torch.float64).index_add_(0, idx, ga.double() + gb.double()).numpy()
    mag = torch.zeros(n_emb, E, dtype=torch.float64).index_add_(0, idx, ga.abs().double() + gb.abs().double()).numpy()
    plain = torch.zeros(n_emb, E).index_add_(0, idx, ga + gb).numpy()
    for name, got in (("torch fp32", plain), ("model", P.model_embed(b))):
        assert_bound(got, ref, mag, c_embed_grad(R), f"embed_grad {name} R={R} n_emb={n_emb}")
