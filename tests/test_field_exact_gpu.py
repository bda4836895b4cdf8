"""emer_field_fwd (field_fwd_kernel<KT0, F>: the neck and the rgb head in one launch) held at kernel level, through the C entry point
(tests/_head_calls.py).

A1 -- exact probes (tests/_head_probe.py has the argument and the builders).  One of the kernel's four GEMM stages is probed at a time
      with the three probe kinds, the other stages copy values exactly: geo / a1 / a2 bitwise the fp64 result, the density within
      C_EXP u of trunc_exp of the exact feature 0, the colours within C_SIG u of the sigmoid of the exact pre-activation.  At 5 rays
      and at 4099 rays of 16 samples: 65 584 rows, three waves of the 256 x 16 take a second ray.
A2 -- bitwise against the separate launches (emer_neck_fwd with 64 outputs, then emer_rgb_head_fwd on its features) on seeded random
      inputs: all eight (KT0, F) instantiations at two level counts each; 1 .. 8195 rays (first, second and third trip of the
      persistent ray loop) of 16 / 48 / 128 samples; Kh = 0 .. 64 and a padded ld_rb; the null a1 / a2 variants; sentinel rows behind
      every output; two launches bitwise equal.

Every tolerance is one the suite already has: bitwise, C_EXP, C_SIG (tests/_bounds.py).
"""
import functools

import numpy as np
import pytest
import torch

from tests import _head_calls as H
from tests import _head_probe as P
from tests._bounds import C_EXP, C_SIG
from tests.test_fused_gpu import NECK_RUNGS
from tests.test_head_exact_gpu import _thin, _trunc_ref

pytestmark = pytest.mark.gpu

OUTS = ("geo", "dens", "a1", "a2", "out")
GRID_RAYS = 256 * 16       # rays of one trip of the persistent loop: persistent_grid(n_rays, 16, 256) workgroups of 16 waves
UNIQUE_ROWS = 4099         # prime: rows i and j of a probe input are equal only if i = j mod 4099, so no two of <= 4099 rays share rows


def _n(t):
    return t.detach().float().cpu().numpy()


# ======================================================================================================== A1: exact probes
STAGES = ("neck0", "neck1", "rgb0", "rgb1")
KH_PROBE = 49
W_JUNK = 123.0             # the per-ray column blocks W0h / W1h of the head's matrices: the kernel must not read them


def _rows(kind, n, cols, seed):
    """n rows of the "b" operand of probe ``kind``: UNIQUE_ROWS distinct rows (the row builder is a Python loop), row i = base[i mod 4099]."""
    base = P.operand_like(kind, min(n, UNIQUE_ROWS), cols, seed, "b")
    return base[np.arange(n) % base.shape[0]]


def _bias(kind, shape, seed):
    """20-bit values on the product grid of probe ``kind`` (some of them zero)."""
    return P.grid_values(np.random.default_rng(seed), shape, 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)


def _copy_neck(K0, seed):
    """Neck weights that make geo = [x_0..31 | +-x_perm(0..31)] of the first 32 input features exactly: unit j holds relu(x_j), unit
    32 + j relu(-x_j), the output layer subtracts the pair.  The other K0 - 32 input features meet zero weights."""
    nw0 = np.zeros((64, K0), np.float32)
    nw0[:, :32] = P.positive_copy(64, 32)
    c = np.concatenate([np.eye(32, dtype=np.float32), P.signed_perm(32, 32, seed)])            # geo = x32 c^T
    nw1 = c @ np.concatenate([np.eye(32, dtype=np.float32), -np.eye(32, dtype=np.float32)], 1)   # x32 = h[:32] - h[32:]
    return nw0, np.zeros(64, np.float32), nw1.astype(np.float32), np.zeros(64, np.float32)


def _probe_inputs(stage, kind, L, Fe, R, S, seed):
    """Every input of emer_field_fwd with ``stage`` probed by ``kind`` and the other stages copying (module docstring)."""
    K0, N = L * Fe, R * S
    zb = np.zeros((R, 64), np.float32)
    copy0 = P.positive_copy(64, 32) @ np.eye(32, 64, dtype=np.float32)     # a1 = relu(+-geo[:, :32])
    copy1a, zero = np.abs(P.signed_perm(64, 64, seed + 4)), np.zeros((64, 64), np.float32)   # a2 = a permutation of a1
    s = dict(w0g=copy0, rb0=zb, w1a=copy1a, w1g=zero, rb1=zb)
    if stage == "neck0":      # layer 0 over the level-major encoding; layer 1 a signed permutation
        s.update(x=_rows(kind, N, K0, seed), nw0=P.operand_like(kind, 64, K0, seed + 1, "a"), nb0=_bias(kind, (64,), seed + 2),
                 nw1=P.signed_perm(64, 64, seed + 3), nb1=np.zeros(64, np.float32))
    elif stage == "neck1":    # layer 0 copies +-x into the hidden units, layer 1 is the probe
        s.update(x=_rows(kind, N, K0, seed), nw0=P.positive_copy(64, K0), nb0=np.zeros(64, np.float32),
                 nw1=P.operand_like(kind, 64, 64, seed + 1, "a"), nb1=_bias(kind, (64,), seed + 2))
    else:
        # the neck copies 32 input features into geo twice, so geo has the probe's activation distribution with twice the non-zeros
        # of x; "lh" / "mm" rows keep 3 non-zeros: geo 6, and in rgb1 a1 (a copy of geo[:, :32]) 3 more share the budget of 2^24 units
        # (9 x 2^20 + a 2^20 bias).  The cover of the probed stage is asserted to be 1.0 below.
        x32 = _rows(kind, N, 32, seed)
        if kind != "hl":
            x32 = _thin(x32, 3)
        extra = np.where(np.arange(N * (K0 - 32)).reshape(N, K0 - 32) % 3 == 0, -1.0, 1.0).astype(np.float32)   # features the neck drops
        nw0, nb0, nw1, nb1 = _copy_neck(K0, seed + 5)
        s.update(x=np.concatenate([x32, extra], 1), nw0=nw0, nb0=nb0, nw1=nw1, nb1=nb1)
        if stage == "rgb0":   # layer 0 over geo plus the per-ray term rb0
            s.update(w0g=P.operand_like(kind, 64, 64, seed + 1, "a"), rb0=_bias(kind, (R, 64), seed + 2))
        else:                 # layer 1 over [a1 | geo] plus rb1
            s.update(w1a=P.operand_like(kind, 64, 64, seed + 1, "a"), w1g=P.operand_like(kind, 64, 64, seed + 6, "a"), rb1=_bias(kind, (R, 64), seed + 2))
    s["w2"] = np.zeros((3, 64), np.float32)
    s["w2"][np.arange(3), [1, 17, 40]] = [1.0, -0.5, 0.25]
    s["b2"] = np.array([0.0, 0.5, -0.25], np.float32)
    return s


def _units_rows(a, b, bias_rows):
    """P.units with a bias per ROW (the per-ray terms): plane magnitudes of b a^T plus |bias| in units of the operands' grid."""
    q = P.grid_of(a) + P.grid_of(b)
    assert P.grid_of(bias_rows) <= q, "bias off the product grid"
    return (P.plane_mag(b) @ P.plane_mag(a).T + np.abs(np.asarray(bias_rows, np.float64))) * 2.0 ** q


def _field_ref(s, S):
    """fp64 forward of the field; per output the entries a correct kernel must return exactly (own sum inside the budget, fed by exact
    entries only -- decided per row, which is conservative)."""
    f = {k: np.asarray(v, np.float64) for k, v in s.items()}
    ray = np.arange(f["x"].shape[0]) // S
    uh = P.units(s["nw0"], s["x"], s["nb0"])
    assert (uh < P.BUDGET).all(), f"probe broken: the neck's hidden layer leaves the exact budget ({uh.max() / P.BUDGET:.2f} x)"
    h = np.maximum(f["x"] @ f["nw0"].T + f["nb0"], 0.0)
    geo = h @ f["nw1"].T + f["nb1"]
    ok_geo = P.units(s["nw1"], h, s["nb1"]) < P.BUDGET
    a1 = np.maximum(geo @ f["w0g"].T + f["rb0"][ray], 0.0)
    ok_a1 = (_units_rows(s["w0g"], geo, f["rb0"][ray]) < P.BUDGET) & ok_geo.all(1, keepdims=True)
    cat, w1 = np.concatenate([a1, geo], 1), np.concatenate([s["w1a"], s["w1g"]], 1)
    a2 = np.maximum(cat @ w1.T.astype(np.float64) + f["rb1"][ray], 0.0)
    ok_a2 = (_units_rows(w1, cat, f["rb1"][ray]) < P.BUDGET) & ok_a1.all(1, keepdims=True)
    z = a2 @ f["w2"].T + f["b2"]
    return dict(geo=(geo, ok_geo), a1=(a1, ok_a1), a2=(a2, ok_a2)), z, ok_a2.all(1)


@pytest.mark.parametrize("R,S", [(5, 16), (GRID_RAYS + 3, 16)])
@pytest.mark.parametrize("L,Fe", [(16, 2), (10, 4)])   # the toy and the shipped encoder: field_fwd_kernel<2, 2> / <3, 4>
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_field_forward_exact(hip_lib, kind, stage, L, Fe, R, S):
    """One stage of emer_field_fwd probed, the others copying.  The probed stage's own output is covered completely (neck0 / neck1:
    geo, rgb0: a1, rgb1: a2; min_cover 1.0); by construction so is everything else (the covers are printed: 1.0 everywhere, the
    thinning of _probe_inputs keeps rgb1's 9 products + bias at <= 10 x 2^20 of the 2^24 units)."""
    N, K0 = R * S, L * Fe
    s = _probe_inputs(stage, kind, L, Fe, R, S, seed=7 * K0 + STAGES.index(stage))
    want, z, row_ok = _field_ref(s, S)
    junk = np.full((64, KH_PROBE), W_JUNK, np.float32)
    c = H.rgb_case(R, S, KH_PROBE, L, Fe, arrays=dict(   # geo: the separate head's input, not read here (a placeholder saves drawing it)
        geo=np.zeros((1, 1), np.float32), enc=np.ascontiguousarray(s["x"].reshape(N, L, Fe).transpose(1, 0, 2)), nw0=s["nw0"], nb0=s["nb0"],
        nw1=s["nw1"], nb1=s["nb1"], rb0=s["rb0"], rb1=s["rb1"], w0=np.concatenate([junk, s["w0g"]], 1),
        w1=np.concatenate([s["w1a"], junk, s["w1g"]], 1), w2=s["w2"], b2=s["b2"]))
    o = H.field_fwd(c)
    own = {"neck0": "geo", "neck1": "geo", "rgb0": "a1", "rgb1": "a2"}[stage]
    tag, cover = f"field {stage} {kind} L{L}F{Fe} R{R}S{S}", {}
    for name, (ref, ok) in want.items():
        assert np.count_nonzero(ref) > ref.size // 128, f"probe broken: {name} is (almost) all zero"
        P.assert_exact(f"{tag} {name}", _n(o[name]), ref, np.where(ok, 0.0, np.inf), min_cover=1.0 if name == own else 0.0, report=cover)
    geo0, ok0 = want["geo"][0][:, 0], want["geo"][1][:, 0]
    P.assert_ulp(f"{tag} density", _n(o["dens"])[ok0], _trunc_ref(geo0[ok0], 0.0)[0], C_EXP)
    P.assert_ulp(f"{tag} colour", _n(o["out"])[row_ok], 1.0 / (1.0 + np.exp(-z[row_ok])), C_SIG)
    cover.update(density=float(ok0.mean()), colour=float(row_ok.mean()))
    print(f"\n[exact] {tag}: cover { {k.split()[-1]: round(v, 3) for k, v in cover.items()} }")


# ================================================================================= A2: bitwise against the separate launches
def _separate(c):
    """emer_neck_fwd (64 outputs, hidden layer not stored) followed by emer_rgb_head_fwd on its features."""
    n = H.neck_fwd(H.neck_of(c), null=("h1",))
    r = H.rgb_head_fwd(c, geo=n["out0"])
    return dict(geo=n["out0"], dens=n["dens"], a1=r["a1"], a2=r["a2"], out=r["out"])


def _assert_same(tag, got, want, skip=()):
    for k in OUTS:
        if k in skip:
            assert got[k] is None
            continue
        assert torch.equal(got[k], want[k]), f"{tag}: {k} differs ({int((got[k] != want[k]).sum())} of {want[k].numel()} entries)"
        assert bool((got[k] != 7.5).reshape(got[k].shape[0], -1).any(1).all()), f"{tag}: rows of {k} were not written"


def _assert_guards(tag, o, guard):
    for k, v in o.items():
        if v is not None:
            g = H.guard_rows(v)
            assert g.shape[0] == guard and bool((g == H.GUARD).all()), f"{tag}: the rows behind {k} were written"


# the odd level count of tests/test_fused_gpu.py::NECK_RUNGS whose features end inside input tile KT0 - 1, and the one that fills the tile
RUNG_LEVELS = [(Lo + d, Fe) for Lo, Fe in NECK_RUNGS if Fe in (2, 4) for d in (0, 1)]
# dispatch_kt0_f<1, 2, 4>: KT0 = ceil(L F / 16) in 1..4 x F in {2, 4}, each with a ragged and a full last tile
assert sorted({(-(-L * Fe // 16), Fe, (L * Fe) % 16 == 0) for L, Fe in RUNG_LEVELS}) == \
    sorted((kt0, Fe, full) for kt0 in (1, 2, 3, 4) for Fe in (2, 4) for full in (False, True))


@pytest.mark.parametrize("L,Fe", RUNG_LEVELS)
def test_field_every_rung(hip_lib, L, Fe):
    """All eight instantiations at (R, S) = (3, 16), with a level count that ends inside the last 16-feature input tile and one that
    fills it."""
    c = H.rgb_case(3, 16, 49, L, Fe)
    _assert_same(f"field L{L}F{Fe}", H.field_fwd(c), _separate(c))


# R: one ray; one workgroup; one ray in a second workgroup; a full grid, no second trip; one / some rays of a second trip; the third trip
SHAPES = [(R, S) for R in (1, 16, 17, GRID_RAYS, GRID_RAYS + 1, 2 * GRID_RAYS + 3) for S in (16, 48, 128) if R * S < 1_000_000]
TWO_RUNGS = [(16, 2), (10, 4)]   # (KT0, F) = (2, 2) and (3, 4)


@pytest.mark.parametrize("L,Fe", TWO_RUNGS)
@pytest.mark.parametrize("R,S", SHAPES)
def test_field_shapes(hip_lib, R, S, L, Fe):
    """Rays from one to three trips of the persistent loop x tiles per ray (the largest case, 4097 x 128, has 524 416 rows;
    8195 x 128 would pass a million and is left out)."""
    c = H.rgb_case(R, S, 49, L, Fe)
    _assert_same(f"field L{L}F{Fe} R{R}S{S}", H.field_fwd(c), _separate(c))


@pytest.mark.parametrize("L,Fe", TWO_RUNGS)
@pytest.mark.parametrize("R,S", [(17, 48), (GRID_RAYS + 1, 16)])
@pytest.mark.parametrize("ld_rb", [128, 132])
@pytest.mark.parametrize("Kh", [0, 17, 48, 49, 64])
def test_field_kh_and_ld_rb(hip_lib, Kh, ld_rb, R, S, L, Fe):
    """The column offsets of W0g / W1a / W1g inside the head's matrices (rgb_views) and the row stride of the per-ray terms.  The pad
    columns of rb hold junk; w0 / w1 are followed by junk rows, so that a view cut one column late still lies inside the allocation."""
    c = H.rgb_case(R, S, Kh, L, Fe, ld_rb=ld_rb, pad_w=True)
    _assert_same(f"field Kh{Kh} ld_rb{ld_rb} L{L}F{Fe} R{R}S{S}", H.field_fwd(c), _separate(c))


@functools.lru_cache(maxsize=2)
def _shared_case(R, S, L, Fe):
    c = H.rgb_case(R, S, 49, L, Fe)
    return c, H.field_fwd(c)


@pytest.mark.parametrize("L,Fe", TWO_RUNGS)
@pytest.mark.parametrize("R,S", [(17, 48), (GRID_RAYS + 1, 16)])
@pytest.mark.parametrize("null", [("a2",), ("a1", "a2")])
def test_field_null_activations(hip_lib, null, R, S, L, Fe):
    """a2 null (the recomputing backward), a1 and a2 null (inference), at several tiles per ray and with a second trip: every other
    output is bitwise that of the call with every pointer given."""
    c, full = _shared_case(R, S, L, Fe)
    _assert_same(f"field null={null} L{L}F{Fe} R{R}S{S}", H.field_fwd(c, null), full, skip=null)


@pytest.mark.parametrize("L,Fe", TWO_RUNGS)
@pytest.mark.parametrize("R", [1, GRID_RAYS + 1])
def test_field_writes_its_rows_only(hip_lib, R, L, Fe):
    """19 sentinel rows behind geo, dens, a1, a2 and out are intact after the call, for every pointer variant."""
    c, full = _shared_case(R, 16, L, Fe)
    for null in ((), ("a2",), ("a1", "a2")):
        o = H.field_fwd(c, null, guard=19)
        _assert_guards(f"field null={null} L{L}F{Fe} R{R}", o, 19)
        _assert_same(f"field (guarded) null={null} L{L}F{Fe} R{R}", o, full, skip=null)


@pytest.mark.parametrize("L,Fe", TWO_RUNGS)
@pytest.mark.parametrize("R,S", [(17, 48), (2 * GRID_RAYS + 3, 16)])
def test_field_two_launches_agree(hip_lib, R, S, L, Fe):
    """The kernel has no atomics: a second launch on the same inputs writes the same bits."""
    c, full = _shared_case(R, S, L, Fe)
    _assert_same(f"field again L{L}F{Fe} R{R}S{S}", H.field_fwd(c), full)
