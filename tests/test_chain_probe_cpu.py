"""The chain probes of tests/_chain_probe.py on the CPU: every probe is inside the exact budget where the GPU file demands
cover 1.0, every kernel branch has a case (decided with the launch-plan restatement), the fp64 executor differs from each
of its three mutants on the cases meant to catch it, and the ``*_supported`` predicates of emernerf_amd.fused agree with
the plan restatement."""
import numpy as np
import pytest

from tests import _chain_probe as C
from tests import _head_probe as P

KINDS = P.KINDS


def _exact_stores(cid, res):
    """(name, value, units) of the stores of a descriptor case that must be exact."""
    out = []
    for k in res:
        if ":" in k:
            continue
        out.append((k, res[k + ":pre"] if cid in ("sigmoid", "trunc_exp") else res[k], None if cid == "fix" else res[k + ":units"]))
    return out


def _all_cases():
    return [("a", k, v) for k, v in C.descriptor_cases().items()] + [("b", k, v) for k, v in C.second_pass_cases().items()]


@pytest.mark.parametrize("kind", KINDS)
def test_descriptor_probes_are_inside_the_budget(kind):
    for grp, cid, build in _all_cases():
        segs, layers, cols, rows = build(kind)
        pl = C.plan_of(segs, layers, cols)
        assert pl["fits"], (cid, pl)
        res = C.accumulate_units(segs, layers, cols, rows, C.run_ref(segs, layers, cols, rows))
        for name, val, un in _exact_stores(cid, res):
            assert np.isfinite(val).all() and np.array_equal(val.astype(np.float32).astype(np.float64), val), (cid, name)
            if un is not None:
                assert (un < P.BUDGET).all(), f"{cid} {kind} {name}: {un.max() / P.BUDGET:.2f} x the budget"
            assert np.count_nonzero(val) > 0 or rows == 1, (cid, name)


def test_every_kernel_branch_has_a_case():
    ntiles, kmod, waves, lmf, multi = set(), set(), set(), set(), 0
    inside = outside = 0
    for grp, cid, build in _all_cases():
        segs, layers, cols, rows = build("lh")
        pl = C.plan_of(segs, layers, cols)
        ntiles |= set(pl["ntiles"])
        kmod |= {C._eff_w(L).shape[1] % 8 for L in layers}
        waves.add(pl["n_waves"])
        multi += rows > pl["rows_per_pass"]
        for S in segs:
            if S["mode"] == 1:
                lmf.add(S["data"].shape[2])
            elif S["row_div"] > 1:
                for row0 in range(0, rows, 16):
                    if row0 % S["row_div"] + 15 < S["row_div"]:
                        outside += 1      # the 16 rows share one source row
                    else:
                        inside += 1       # a ray boundary inside the tile
        lmf |= {L["store_lm"] for L in layers if L["store_lm"]}
        if grp == "b":
            assert rows == pl["rows_per_pass"] + 17
    assert ntiles >= {1, 2, 3, 4, 5, 8, 16}, ntiles
    assert kmod >= {0, 1, 4, 7}, kmod
    assert min(waves) < 16 and max(waves) == 16, waves
    assert multi >= 2 and inside and outside
    assert lmf >= {1, 2, 3, 4, 8}, lmf
    b = C.second_pass_cases()
    assert C.plan_of(*b["narrow"]("lh")[:3])["n_waves"] == 16 and C.plan_of(*b["wide"]("lh")[:3])["n_waves"] < 16


def _differs(a, b, keys):
    return any(not np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _skip_forward_desc(H, K0, Cc, rows, in_place, kind="lh", probed=1):
    """The forward descriptor of the skip heads on probe values: A2 over A1 (the layout before the fix) or in columns of its own."""
    x, (w0, b0, w1, b1, w2, b2) = C.skip_probe(kind, probed, H, K0, Cc, rows, seed=5)
    c_x = H
    c_e = c_x + C._r4(K0)
    c_a2 = 0 if in_place else c_e
    c_o = c_e if in_place else c_e + H
    return ([C.rm(x, c_x)], [C.lay(w0, b0, c_x, 0, C.ACT_RELU, store="a1"), C.lay(w1, b1, 0, c_a2, C.ACT_RELU, store="a2"),
                              C.lay(w2, b2, c_a2, c_o, store="out")], c_o + C._r4(Cc), rows)


def test_reference_differs_from_each_mutant():
    # column groups: the in-place A2 of a 96-wide skip head is the overlap; with A2 in its own columns nothing overlaps
    d = _skip_forward_desc(96, 27, 3, 33, in_place=True)
    assert _differs(C.run_ref(*d), C.run_ref(*d, mutant="overlap"), ("a2", "out"))
    d = _skip_forward_desc(96, 27, 3, 33, in_place=False)
    assert not _differs(C.run_ref(*d), C.run_ref(*d, mutant="overlap"), ("a1", "a2", "out"))
    # the in-place layout of a 64-wide head is one column group: legal
    d = _skip_forward_desc(64, 27, 3, 33, in_place=True)
    assert not _differs(C.run_ref(*d), C.run_ref(*d, mutant="overlap"), ("a1", "a2", "out"))
    # K % 8 tails: every case with a tail on a probed layer
    n = 0
    for grp, cid, build in _all_cases():
        d = build("lh")
        if any(C._eff_w(L).shape[1] % 8 for L in d[1]) and d[3] > 1:
            keys = [k for k in C.run_ref(*d) if ":" not in k]
            assert _differs(C.run_ref(*d), C.run_ref(*d, mutant="drop_tail"), keys), cid
            n += 1
    assert n >= 10
    # accumulate: the single-pass case (previous tile = none) and both second-pass cases (previous tile = the first pass)
    d = C.accumulate_case("lh")
    assert _differs(C.run_ref(*d), C.run_ref(*d, mutant="acc_prev"), ("y",))
    for cid, build in C.second_pass_cases().items():
        d = build("lh")
        rpp = C.plan_of(*d[:3])["rows_per_pass"]
        a, m = C.run_ref(*d)["y"], C.run_ref(*d, mutant="acc_prev")["y"]
        assert not np.array_equal(a[rpp:], m[rpp:]), cid


def _density_desc(H, rows, c_o_of, rpp):
    """density_mlp's slow-branch forward on values whose first ``rpp`` rows overflow the density (pre-activation 100)."""
    K0 = 7
    x = np.zeros((rows, K0), np.float32); x[:, 0] = 1.0
    x[rpp:, 0] = 0.5
    w0 = P.positive_copy(H, K0)
    w1 = np.zeros((1, H), np.float32); w1[0, 0] = 100.0
    enc = np.ascontiguousarray(x.reshape(rows, K0, 1).transpose(1, 0, 2))
    c_h = C._r4(K0)
    c_o = c_o_of(c_h, H)
    return ([C.lm(enc, 0)], [C.lay(w0, np.zeros(H, np.float32), 0, c_h, C.ACT_RELU, store="h"),
                             C.lay(w1, np.zeros(1, np.float32), c_h, c_o, C.ACT_TRUNC_EXP, store="dens")], c_o + 4, rows)


def test_stale_buffer_model_shows_the_inf_hazard_and_its_fix():
    """The kernel's buffer model (``stale``): with the output column inside layer 1's K % 8 padding an overflowed density of
    the previous tile turns the next tile into NaN; past the padding (fused.density_mlp's layout) it cannot."""
    from emernerf_amd import fused
    rpp = 64
    for H in (20, 28, 128):
        old = _density_desc(H, rpp + 17, lambda c_h, H: c_h + C._r4(H), rpp)
        new = _density_desc(H, rpp + 17, lambda c_h, H: c_h + C._ru(H, 8), rpp)
        assert new[2] == fused.density_mlp_chain_shapes(7, H)[0][0]
        want = C.run_ref(*new, rows_per_pass=rpp)["dens"]
        assert np.isinf(want[:rpp]).all() and np.isfinite(want[rpp:]).all()
        got_new = C.run_ref(*new, stale=True, rows_per_pass=rpp)["dens"]
        assert np.array_equal(got_new, want), H
        got_old = C.run_ref(*old, stale=True, rows_per_pass=rpp)["dens"]
        assert np.isnan(got_old[rpp:]).all() == (H % 8 != 0), H


def test_supported_predicates_agree_with_the_plan():
    from emernerf_amd import fused

    def fits4(shapes):
        ok = True
        for cols, kn in shapes:
            pl = C.plan(cols, kn)
            ok &= cols <= C.MAX_COLS and pl["lds4"] <= C.LDS_BYTES
            assert pl["fits"] == (cols <= C.MAX_COLS and pl["lds4"] <= C.LDS_BYTES)   # the kernel never goes below 4 waves
        return ok

    n_true = n_false = 0
    for H in (20, 32, 64, 96, 128, 256):
        for Kx in (17, 27, 43, 70, 113):
            for Cc in (1, 3, 20):
                got = fused.skip_mlp3_supported(H, Kx, Cc)
                assert got == fits4(fused.skip_mlp3_chain_shapes(H, Kx, Cc)), (H, Kx, Cc)
                n_true += got; n_false += not got
                for NG in (32, 64):
                    got = fused.rgb_head_supported(H, Kx, NG, Cc)
                    assert got == fits4(fused.rgb_head_chain_shapes(H, Kx, NG, Cc)), (H, Kx, NG, Cc)
                    n_true += got; n_false += not got
            for NG in (16, 64, 80, 128):
                got = fused.base_mlp_supported(Kx, H, NG)
                assert got == fits4(fused.base_mlp_chain_shapes(Kx, H, NG)), (H, Kx, NG)
            assert fused.density_mlp_supported(Kx, H) == fits4(fused.density_mlp_chain_shapes(Kx, H))
    assert n_true > 20 and n_false > 20
    assert not fused.rgb_head_supported(256, 49, 64, 3) and not fused.skip_mlp3_supported(256, 43, 3)
    assert not fused.base_mlp_supported(32, 512, 128) and not fused.density_mlp_supported(480, 64)
    assert fused.rgb_head_supported(64, 49, 64, 3) and fused.skip_mlp3_supported(64, 43, 3)      # the shipped shapes
    # the layouts the Functions use: a skip head wider than 64 has A2 in columns of its own, a narrower one in place
    assert fused._skip_cols(64, 113, 3) == (64, 0, 180, 184) and fused._skip_cols(96, 27, 3) == (96, 124, 220, 224)
    for dims in C.SEQ_CASES:
        import torch
        ws = [torch.empty(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]
        assert fused.seq_mlp_supported(ws) == fits4(fused.seq_mlp_chain_shapes(list(dims))) == (dims in C.SEQ_CHAIN), dims


# ------------------------------------------------------------------------------------------------------------ Function level
@pytest.mark.parametrize("kind", KINDS)
def test_skip_head_probes_cover(kind):
    """Forward inside the budget (skip_ref asserts it per layer) and, for skip_mlp3, pass-A dx exact on every row and the probed
    layer's dW / db exact under pass B."""
    from tests.test_head_exact_gpu import _seeds
    for H, K0, Cc, rows in C.SKIP_CASES:
        for probed in (0, 1, 2):
            x, ws = C.skip_probe(kind, probed, H, K0, Cc, rows, seed=H + K0 + probed)
            ref = C.skip_ref(x, ws)
            g = _seeds(kind, rows, Cc, rows + probed)
            assert C.skip_ref_bwd(x, ws, ref, g["A"])["ok"].all(), (H, K0, Cc, probed)
            bw = C.skip_ref_bwd(x, ws, ref, g["B"])
            assert bw[f"dW{probed}"][1].all() and bw[f"db{probed}"][1].all(), (H, K0, Cc, probed)
            assert np.count_nonzero(ref["a2"]) and np.count_nonzero(ref["z"])
    for H, Kh, NG, Cc, R, S in C.RGB_CASES:
        for probed in (0, 1, 2):
            _, _, x = C.rgb_rows(kind, R, S, Kh, NG, seed=H + Kh)
            x, ws = C.skip_probe(kind, probed, H, Kh + NG, Cc, R * S, seed=H + Kh + probed, x=x)
            ref = C.skip_ref(x, ws)
            assert np.count_nonzero(ref["a2"]) and np.count_nonzero(ref["z"])


def stack_cases():
    """(tag, widths, rows) of the plain stacks: base_mlp / density_mlp necks (two layers) and the seq_mlp stacks."""
    out = [(f"base L{L}F{F}", (L * F, H, NG), rows) for L, F, H, NG, rows in C.BASE_CASES]
    return out + [(f"seq {d}", d, C.SEQ_ROWS) for d in C.SEQ_CASES]


@pytest.mark.parametrize("kind", KINDS)
def test_stack_probes_cover(kind):
    """base_mlp and seq_mlp stacks: forward 1.0 (mlp_ref asserts), pass-A dx 1.0, the probed layer's dW / db 1.0 under pass B."""
    from tests.test_head_exact_gpu import _seeds, _stack
    for tag, widths, rows in stack_cases():
        n = len(widths) - 1
        relus = [True] * (n - 1) + [False]
        for layer in range(n):
            x, Ws, Bs = _stack(kind, layer, widths, rows, seed=sum(widths) + layer)
            hs, pres = P.mlp_ref(x, Ws, Bs, relus)
            for pas, g in _seeds(kind, rows, widths[-1], seed=rows + layer).items():
                want = P.mlp_ref_bwd(hs, pres, Ws, relus, g)
                must = ("dx",) if pas == "A" else (f"dW{layer}", f"db{layer}")
                for m in must:
                    assert want[m][1].all(), f"{tag} {kind} layer {layer} pass {pas}: {m} cover {want[m][1].mean():.3f}"
