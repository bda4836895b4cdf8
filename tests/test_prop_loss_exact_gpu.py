"""emer_prop_loss (csrc/proploss.hip) held to exact probes and per-entry fp64 bounds (tests/_prop_probe.py has the
argument, the builders and the references; tests/test_prop_loss_bounds_cpu.py shows what they catch).

* exact probes, both modes: dyadic inputs make every intermediate up to the hinge argument exact, so a gradient entry is
  exactly 0 where the hinge is inactive on both sides and otherwise within c_prop_grad u (|G_{j-1}| + |G_j|) scale of the
  fp64 reference, a per-ray loss within c_prop_ray_loss u of itself and the total the double sum of the per-ray values
  rounded once.  Through the entry point directly (per-ray buffer) and through ops.prop_level_loss;
* inputs shaped like a training step (empty space, thin walls, saturation; final edges importance-sampled) at the shipped
  pulses: every entry inside the first-order bound of tests/_bounds.prop_aa_bound, none excluded;
* what the entry point promises about its arguments.
"""
import numpy as np
import pytest
import torch

from tests import _prop_probe as P
from tests._bounds import U, C_PROP_TOTAL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SCALE = 2.0 ** -3


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)


def _launch(b, pulse, aa, scale, want_grad=True, accumulate=0, loss_init=float("nan"), rays_buf=True):
    """emer_prop_loss called directly: (loss_rays [R], loss_out, d_cdf_prop [R, m+1] or None) as numpy.  Every output
    buffer is pre-filled with NaN (loss_out with ``loss_init``): an entry the launch does not write shows."""
    from emernerf_amd import _lib
    from emernerf_amd.ops import _ptr, _stream
    sf, tr, sp, cp = _d(b["s_fin"]), _d(b["trans"]), _d(b["s_p"]), _d(b["c_p"])
    R, n = tr.shape
    m = cp.shape[1] - 1
    rays = torch.full((max(R, 1),), float("nan"), device=DEV)
    loss = torch.full((1,), loss_init, device=DEV)
    dcp = torch.full((max(R, 1), m + 1), float("nan"), device=DEV) if want_grad else None
    _lib.call("emer_prop_loss", _ptr(sf), _ptr(tr), n, _ptr(sp), _ptr(cp), m, float(pulse), int(aa), R, float(scale),
              _ptr(rays) if rays_buf else None, _ptr(loss) if rays_buf else None, int(accumulate), _ptr(dcp), _stream(tr))
    torch.cuda.synchronize()
    return rays[:R].cpu().numpy(), loss.cpu().numpy()[0], None if dcp is None else dcp[:R].cpu().numpy()


def _assert_total(loss_out, rays, what, prev=0.0):
    """The reduction accumulates in double: loss_out is the double sum (+ the previous value) rounded once."""
    want = float(np.asarray(rays, np.float64).sum()) + float(prev)
    assert abs(float(loss_out) - want) <= C_PROP_TOTAL * U * abs(want), f"{what}: total {loss_out!r} vs double sum {want!r}"


def _through_wrapper(b, pulse, aa, scale, upstream):
    from emernerf_amd import ops
    cd = _d(b["c_p"]).requires_grad_(True)
    loss = ops.prop_level_loss(_d(b["s_fin"]), _d(b["trans"]), _d(b["s_p"]), cd, pulse, aa, scale)
    (loss * upstream).backward()
    return loss.detach().cpu().numpy(), cd.grad.cpu().numpy()


@pytest.mark.parametrize("shape", P.SHAPES)
@pytest.mark.parametrize("family", P.FAMILIES)
def test_probes_exact(hip_lib, family, shape):
    """Mode 0 on every probe family, R = 1, 4 and 13 rays (the last workgroup has one live wave)."""
    n, m = shape
    for R in P.RAYS:
        ref = P.probe_reference(R, n, m, family, R % 2, SCALE)
        b = ref[0]
        what = f"{family} n={n} m={m} R={R} pulse=2^{int(np.log2(b['pulse']))}"
        rays, total, grad = _launch(b, b["pulse"], 1, SCALE)
        P.check_aa_outputs(ref, SCALE, rays, grad, what)
        _assert_total(total, rays, what)
        wl, wg = _through_wrapper(b, b["pulse"], True, SCALE, 0.5)   # (a power of two upstream: exact)
        assert wl.view(np.uint32) == np.float32(total).view(np.uint32), f"{what}: ops.prop_level_loss returns another total"
        assert np.array_equal(wg, grad * np.float32(0.5)), f"{what}: ops.prop_level_loss returns another gradient"


@pytest.mark.parametrize("shape", P.SHAPES + ((100, 4),))
@pytest.mark.parametrize("kind", ("shared", "scatter", "mixed"))
def test_pdf_probes_exact(hip_lib, kind, shape):
    """Mode 1: final edges equal to proposal edges, many final intervals scattering into one entry (the bound carries the
    hit count and the abs-sum: the order of the LDS atomics is free)."""
    n, m = shape
    for R in P.RAYS:
        ref = P.pdf_reference(R, n, m, kind, R % 2, SCALE)
        b = ref[0]
        what = f"pdf {kind} n={n} m={m} R={R}"
        rays, total, grad = _launch(b, 0.0, 0, SCALE)
        P.check_pdf_outputs(ref, SCALE, rays, grad, what)
        _assert_total(total, rays, what)
        wl, wg = _through_wrapper(b, 0.0, False, SCALE, 0.5)
        assert wl.view(np.uint32) == np.float32(total).view(np.uint32)
        P.check_pdf_outputs(ref, SCALE, rays, wg * 2.0, what + " (wrapper)")   # (atomics: not bitwise the direct call's)


REAL_SHAPES = [(13, 128, 128, 0), (13, 128, 64, 1), (5, 48, 64, 0), (5, 900, 512, 0)]   # the last: 162 576 B of LDS of 160 KiB


@pytest.mark.parametrize("R,n,m,level", REAL_SHAPES)
def test_realistic_inputs_inside_the_bound(hip_lib, oracle, R, n, m, level):
    """Training-like rays at the shipped pulses, every gradient entry and per-ray loss inside the first-order fp64 bound.
    Measured on an MI355X, worst err / bound in the order of REAL_SHAPES: gradient 0.019, 0.158, 0.060, 0.0036; per-ray
    loss 0.0015, 0.020, 0.0031, 5.5e-5 (the numpy model's figures to the printed digits; DESIGN.md 4.4 has the medians)."""
    scale = 1024.0 / (R * m)
    ref = P.realistic_reference(R, n, m, level, 7 + n + m, scale, oracle)
    b, pulse = ref[0], ref[1]
    what = f"R={R} n={n} m={m} pulse={pulse:.4f}"
    rays, total, grad = _launch(b, pulse, 1, scale)
    P.check_realistic_outputs(ref, rays, grad, f"kernel {what}")
    _assert_total(total, rays, what)
    wl, wg = _through_wrapper(b, pulse, True, scale, 1.0)
    assert wl.view(np.uint32) == np.float32(total).view(np.uint32) and np.array_equal(wg, grad)


# -------------------------------------------------------------------------------------------------- argument handling
def _small(R=3, n=16, m=12):
    return P.probe_reference(R, n, m, "zero_wp", 0, SCALE)[0]


def _zeros(R, n, m):
    return dict(s_fin=np.tile(np.linspace(0, 1, n + 1, dtype=np.float32), (R, 1)), trans=np.ones((R, n), np.float32),
                s_p=np.tile(np.linspace(0, 1, m + 1, dtype=np.float32), (R, 1)), c_p=np.tile(np.linspace(0, 1, m + 1, dtype=np.float32), (R, 1)))


@pytest.mark.parametrize("n,m,pulse,aa", [(1100, 512, 0.03, 1), (2049, 16, 0.03, 1), (16, 513, 0.03, 1), (1100, 512, 0.0, 0),
                                          (16, 16, 0.0, 1), (16, 16, -0.03, 1)])
def test_rejected_arguments_launch_nothing(hip_lib, n, m, pulse, aa):
    """Beyond the LDS limit (9 (n + 1) + 4 (m + 1) floats per ray, four rays per workgroup, 160 KiB), n_final > 2048,
    n_prop > 512, a non-positive pulse in the anti-aliased mode: EmerError, and no output buffer is touched."""
    from emernerf_amd import _lib
    b = _zeros(1, n, m)
    sf, tr, sp, cp = _d(b["s_fin"]), _d(b["trans"]), _d(b["s_p"]), _d(b["c_p"])
    from emernerf_amd.ops import _ptr, _stream
    rays, loss, dcp = torch.full((1,), 7.5, device=DEV), torch.full((1,), 7.5, device=DEV), torch.full((1, m + 1), 7.5, device=DEV)
    with pytest.raises(_lib.EmerError):
        _lib.call("emer_prop_loss", _ptr(sf), _ptr(tr), n, _ptr(sp), _ptr(cp), m, float(pulse), aa, 1, 1.0, _ptr(rays), _ptr(loss), 0,
                  _ptr(dcp), _stream(tr))
    torch.cuda.synchronize()
    assert float(rays[0]) == 7.5 and float(loss[0]) == 7.5 and bool((dcp == 7.5).all()), "a rejected call wrote to its outputs"


def test_admitted_limit_is_admitted(hip_lib):
    """n = 900, m = 512 is inside every limit (REAL_SHAPES runs it on real inputs); the pdf mode at the same shape too."""
    b = _zeros(2, 900, 512)
    rays, total, grad = _launch(b, 0.0, 0, 1.0)
    assert np.isfinite(rays).all() and np.isfinite(grad).all() and np.isfinite(total)


def test_no_rays(hip_lib):
    b = _small()
    empty = {k: v[:0] for k, v in b.items() if k in ("s_fin", "trans", "s_p", "c_p")}
    _, total, _ = _launch(empty, b["pulse"], 1, SCALE, loss_init=3.25)
    assert total == 0.0, "n_rays = 0 without accumulate must zero loss_out"
    _, total, _ = _launch(empty, b["pulse"], 1, SCALE, loss_init=3.25, accumulate=1)
    assert total == 3.25, "n_rays = 0 with accumulate must leave loss_out as it was"


@pytest.mark.parametrize("aa", [1, 0])
def test_accumulate_no_gradient_and_determinism(hip_lib, aa):
    ref = P.probe_reference(13, 48, 40, "zero_wp", 1, SCALE) if aa else P.pdf_reference(13, 48, 40, "mixed", 1, SCALE)
    b = ref[0]
    pulse = b["pulse"] if aa else 0.0
    rays, total, grad = _launch(b, pulse, aa, SCALE)
    assert np.isfinite(rays).all() and np.isfinite(grad).all() and total > 0
    # accumulate = 1 adds to the previous value: the double sum rounded once
    prev = float(np.float32(1234.56789))
    rays_a, total_a, _ = _launch(b, pulse, aa, SCALE, accumulate=1, loss_init=prev)
    assert np.array_equal(rays_a, rays)
    _assert_total(total_a, rays, "accumulate", prev=prev)
    assert total_a != total
    # no gradient buffer: the loss is bitwise unchanged
    rays_n, total_n, none = _launch(b, pulse, aa, SCALE, want_grad=False)
    assert none is None and np.array_equal(rays_n, rays) and np.float32(total_n).view(np.uint32) == np.float32(total).view(np.uint32)
    # only the gradient: no loss buffers
    _, _, grad_only = _launch(b, pulse, aa, SCALE, rays_buf=False)
    # two runs: bitwise equal loss and per-ray values; the gradient too in mode 0 (mode 1: LDS atomics, no fixed order)
    rays2, total2, grad2 = _launch(b, pulse, aa, SCALE)
    assert np.array_equal(rays2, rays) and np.float32(total2).view(np.uint32) == np.float32(total).view(np.uint32)
    if aa:
        assert np.array_equal(grad2.view(np.uint32), grad.view(np.uint32)) and np.array_equal(grad_only.view(np.uint32), grad.view(np.uint32))
    else:
        P.check_pdf_outputs(ref, SCALE, rays2, grad_only, "pdf, gradient only")
