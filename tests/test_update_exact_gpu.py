"""The update kernels of csrc/elementwise.hip on the device against the probes and bounds of tests/_update_probe.py and
tests/_bounds.py (whose own power tests/test_update_bounds_cpu.py shows without a GPU): emer_adam_step (vector kernel with its
head / body / tail split, the capped grid's second trip, the scalar kernel), emer_contract_bwd, emer_flow_warp_fwd / bwd,
emer_cast_f32_f16, and the second grid-stride trip of emer_aggregate3 / emer_aggregate3_density.

Every buffer a kernel writes sits between guards of at least ``P.GUARD`` sentinel NaNs that must come back with their bits;
pure outputs are handed over filled with the same sentinel.  Shapes are the smallest that reach the path they name:
STREAM = 524 288 threads is the cap of every streaming grid (stream_blocks: 2048 blocks of 256), so N = STREAM + 257 is the
smallest row count whose loop takes a second trip with a partial last block.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _update_probe as P

pytestmark = pytest.mark.gpu

F32 = np.float32
STREAM = P.STREAM_THREADS
FRONT = 12             # floats in front of a guarded fp32 buffer: >= P.GUARD, and a multiple of 4 so that the data keeps its 16-byte phase
FRONT_F16 = 16         # halves in front of the cast's destination (which must be 16-byte aligned)
assert FRONT >= P.GUARD and FRONT_F16 >= P.GUARD


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Guarded:
    """An fp32 device buffer [FRONT + phase sentinels | data | GUARD sentinels]; ``phase`` floats move the data's start behind a
    16-byte boundary.  data = None hands the kernel a pure output: sentinels throughout."""

    def __init__(self, n, data=None, phase=0):
        self.front, self.n = FRONT + phase, n
        host = P.sentinel(self.front + n + P.GUARD)
        if data is not None:
            host[self.front:self.front + n] = np.asarray(data, F32).reshape(-1)
        self.buf = torch.from_numpy(host).to(_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.front:self.front + n]
        assert self.view.data_ptr() % 16 == 4 * (phase % 4)

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert P.is_sentinel(host[:self.front]) and P.is_sentinel(host[self.front + self.n:]), f"{what}: a guard was overwritten"
        return host[self.front:self.front + self.n]


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _run_adam(b, phases, what, report=None):
    """One ops.adam_step on guarded views of the build's state; phases = the 16-byte phase (in floats) of p, g, m, v."""
    from emernerf_amd import ops
    hp = b["hp"]
    bufs = [Guarded(b["n"], b[k], ph) for k, ph in zip("pgmv", phases)]
    g0 = bufs[1].buf.clone()
    ops.adam_step(*(x.view for x in bufs), hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["gs"], hp["step"])
    p, m, v = (bufs[i].result(f"{what} {'pgmv'[i]}") for i in (0, 2, 3))
    assert torch.equal(bufs[1].buf.view(torch.int32), g0.view(torch.int32)), f"{what}: the gradient buffer was written"
    P.check_adam(b, p, m, v, what, report)


# ------------------------------------------------------------------------------------------------------------------- Adam
# (off, step, wd, gs): every value of off {0..3} x step {1, 7, 25000} x wd {1e-5, 0} x gs {1/1024, 1} three times or more
ADAM_RANDOM = [(0, 1, 1e-5, 1 / 1024), (1, 7, 1e-5, 1 / 1024), (2, 25000, 1e-5, 1 / 1024), (3, 1, 0.0, 1 / 1024), (0, 7, 0.0, 1.0), (1, 25000, 1e-5, 1.0),
               (2, 1, 1e-5, 1.0), (3, 7, 1e-5, 1 / 1024), (0, 25000, 0.0, 1 / 1024), (1, 1, 0.0, 1.0), (2, 7, 0.0, 1 / 1024), (3, 25000, 0.0, 1.0)]
ADAM_N = 100_003


@pytest.mark.parametrize("off,step,wd,gs", ADAM_RANDOM)
def test_adam_random_family_is_inside_the_bounds(hip_lib, off, step, wd, gs):
    """m', v' and p' of one step, every entry inside adam_bounds (head of (4 - off) % 4, 25 000 vectors, a tail)."""
    hp = dict(P.ADAM_HP, step=step, wd=wd, gs=gs)
    _run_adam(P.build_adam_random(ADAM_N, hp), (off,) * 4, f"adam n={ADAM_N} off={off} step={step} wd={wd} gs={gs:.3g}")


@pytest.mark.parametrize("variant,off", [("base", 0), ("base", 1), ("wd0", 2), ("gs1", 3), ("wd0", 1), ("gs1", 0), ("base", 3), ("gs1", 2)])
def test_adam_exact_probes(hip_lib, variant, off):
    _run_adam(P.build_adam_exact(ADAM_N, variant), (off,) * 4, f"adam exact {variant} off={off}")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_adam_tiny_slices(hip_lib, off):
    """n in {1 .. 9}: head > n (clamped), no body, head plus tail only, one body vector with and without a tail."""
    for n in (1, 2, 3, 4, 5, 7, 8, 9):
        for variant in P.ADAM_EXACT_VARIANTS:
            _run_adam(P.build_adam_exact(n, variant), (off,) * 4, f"adam exact {variant} n={n} off={off}")
        for step, wd, gs in ((1, 1e-5, 1 / 1024), (7, 0.0, 1.0)):
            _run_adam(P.build_adam_random(n, dict(P.ADAM_HP, step=step, wd=wd, gs=gs)), (off,) * 4, f"adam n={n} off={off} step={step}")


def test_adam_capped_grid_second_trip(hip_lib):
    """off = 1 and n = 4 (3 STREAM + 300) + 3 + 2: the grid is capped at STREAM threads of two vectors per trip, so the body's
    second trip runs with both vectors for 300 threads and with one elsewhere, behind a 3-element head and before a 2-element tail."""
    n = 4 * (3 * STREAM + 300) + 3 + 2
    assert n == 6_292_661 and P.adam_split(n, 1) == (3, 3 * STREAM + 300, n - 2)
    _run_adam(P.build_adam_random(n, dict(P.ADAM_HP, step=7)), (1,) * 4, f"adam n={n} off=1 step=7")


@pytest.mark.parametrize("n", [1000, STREAM + 257])
def test_adam_scalar_kernel(hip_lib, n):
    """The four arrays at different 16-byte phases: adam_scalar_kernel; n = STREAM + 257 is its own second trip."""
    _run_adam(P.build_adam_random(n, dict(P.ADAM_HP, step=7)), (0, 1, 2, 3), f"adam scalar n={n}")
    _run_adam(P.build_adam_exact(n, "base"), (3, 0, 2, 1), f"adam scalar exact n={n}")


def test_adam_step_rejects_bad_arguments(hip_lib, monkeypatch):
    """Anything but four fp32, contiguous, equally long tensors on one device is an error, and no kernel is launched on them."""
    from emernerf_amd import _lib, ops
    dev = _dev()
    n = 64
    good = [torch.zeros(n, device=dev) for _ in range(4)]
    calls = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: calls.append(a[0]))
    args = (0.01, 0.9, 0.99, 1e-15, 1e-5, 1.0, 1)
    bad = {"float16": torch.zeros(n, device=dev, dtype=torch.float16), "float64": torch.zeros(n, device=dev, dtype=torch.float64),
           "strided": torch.zeros(2 * n, device=dev)[::2], "short": torch.zeros(n - 1, device=dev), "long": torch.zeros(n + 1, device=dev),
           "cpu": torch.zeros(n)}
    for i in range(4):
        for name, t in bad.items():
            a = list(good)
            a[i] = t
            with pytest.raises(_lib.EmerError):
                ops.adam_step(*a, *args)
            assert not calls, f"argument {i} {name}: a kernel was launched"
    ops.adam_step(*good, *args)
    assert calls == ["emer_adam_step"]


# ------------------------------------------------------------------------------------------------------------ contraction
@pytest.mark.parametrize("N", [1, 37, STREAM + 257])
@pytest.mark.parametrize("unbounded", [True, False])
def test_contract_bwd(hip_lib, N, unbounded):
    from emernerf_amd import _lib
    for b in (P.build_contract_exact(N, unbounded), P.build_contract_random(N, unbounded)):
        what = f"contract_bwd {'exact' if b['exact'] else 'random'} N={N} unbounded={unbounded}"
        out = Guarded(3 * N)
        pos, aabb, g = _t(b["pos"]), _t(b["aabb"]), _t(b["g"])
        _lib.call("emer_contract_bwd", _ptr(pos), _ptr(aabb), int(unbounded), _ptr(g), _ptr(out.view), N, _stream())
        P.check_contract_bwd(b, out.result(what).reshape(N, 3), what)


# -------------------------------------------------------------------------------------------------------------- flow warp
@pytest.mark.parametrize("N", [37, STREAM + 257])
@pytest.mark.parametrize("unbounded", [True, False])
@pytest.mark.parametrize("exact", [True, False])
def test_flow_warp(hip_lib, N, unbounded, exact):
    """Forward bit for bit against the fp32 model (rows where both time clamps bind and rows with noise == 0 included);
    backward against restate_flow_warp_bwd, exact on the probes and inside flow_warp_bwd_bounds on the random family, for dx3
    alone, dx2 alone and both."""
    from emernerf_amd import _lib
    for b in (P.build_flow(N, unbounded, exact),):
        what = f"flow_warp {'exact' if b['exact'] else 'random'} N={N} unbounded={unbounded}"
        pos, nrm, ts, fl, nz, aabb = (_t(b[k]) for k in ("pos", "normed", "ts", "flow", "noise", "aabb"))
        x3, x2 = Guarded(12 * N), Guarded(8 * N)
        _lib.call("emer_flow_warp_fwd", _ptr(pos), _ptr(nrm), _ptr(ts), _ptr(fl), _ptr(nz), float(b["dt"]), _ptr(aabb), int(unbounded), _ptr(x3.view),
                  _ptr(x2.view), N, _stream())
        P.check_flow_fwd(b, x3.result(f"{what} x3"), x2.result(f"{what} x2"), what)
        for which in P.FLOW_CONSUMERS:
            d3, d2 = (_t(x) for x in P.flow_grads(b, which))
            out = Guarded(6 * N)
            _lib.call("emer_flow_warp_bwd", _ptr(pos), _ptr(fl), _ptr(nz), _ptr(aabb), int(unbounded), _ptr(d3), _ptr(d2), _ptr(out.view), N, _stream())
            P.check_flow_bwd(b, which, out.result(f"{what} dflow").reshape(N, 6), what)


# ------------------------------------------------------------------------------------------------------------------- cast
def test_cast_f32_f16_is_round_to_nearest_even(hip_lib):
    """Every finite half, every midpoint and its fp32 neighbours, the overflow threshold, the subnormal range (tests/_update_probe.
    cast_sources), with the source 0 .. 3 floats behind a 16-byte boundary (vector loads / scalar loads) and n cut to every
    residue mod 8, n < 8 included: bit for bit numpy's astype(float16), NaN as NaN; nothing past n is written."""
    from emernerf_amd import _lib
    src = P.cast_sources()
    total = src.size
    dsrc = _t(src)
    assert dsrc.data_ptr() % 16 == 0
    dst = torch.empty(FRONT_F16 + total + P.GUARD, device=_dev(), dtype=torch.int16)
    for start in range(4):
        for n in list(range(1, 8)) + [total - start - j for j in range(8)]:
            dst.fill_(P.SENTINEL_F16)
            _lib.call("emer_cast_f32_f16", _ptr(dsrc[start:]), _ptr(dst[FRONT_F16:]), n, _stream())
            host = dst.cpu().numpy().view(np.uint16)
            what = f"cast start={start} n={n}"
            assert (host[:FRONT_F16] == P.SENTINEL_F16).all() and (host[FRONT_F16 + n:] == P.SENTINEL_F16).all(), f"{what}: written outside [0, n)"
            P.check_cast(src[start:start + n], host[FRONT_F16:FRONT_F16 + n], what)
    assert {(total - s - j) % 8 for s in range(1) for j in range(8)} == set(range(8))


# ------------------------------------------------------------------------------------- second trip of the float4 streams
AGG_ROWS, AGG_COLS = 32_800, 64


def test_aggregate3_second_trip(hip_lib):
    """n4 = 32 800 x 16 = 524 800 float4 per third > STREAM: the last 512 take the loop's second trip."""
    from emernerf_amd import ops
    assert AGG_ROWS * AGG_COLS // 4 > STREAM
    g = torch.Generator().manual_seed(5)
    x3 = torch.randn(3 * AGG_ROWS, AGG_COLS, generator=g).to(_dev()).requires_grad_(True)
    out = ops.aggregate3(x3)
    cur, fwd, bwd = x3.detach().split(AGG_ROWS, dim=0)
    assert torch.equal(out, (cur + 0.5 * fwd + 0.5 * bwd) / 2.0)
    up = torch.randn(AGG_ROWS, AGG_COLS, generator=g).to(_dev())
    (dx,) = torch.autograd.grad(out, x3, up)
    assert torch.equal(dx, torch.cat([up / 2.0, 0.5 * (up / 2.0), 0.5 * (up / 2.0)], 0))


def test_aggregate3_density_second_trip(hip_lib):
    """The same size through the kernel pair that also reads the density off column 0: features bit for bit, density =
    expf(f0 - 1) within C_EXP u of exp of the fp32 f0 - 1, backward [h | h / 2 | h / 2] with h = (g + gd dens e_0) / 2."""
    from emernerf_amd import ops
    from tests._bounds import C_EXP
    from tests._head_probe import assert_ulp
    g = torch.Generator().manual_seed(6)
    x3 = torch.randn(3 * AGG_ROWS, AGG_COLS, generator=g).to(_dev()).requires_grad_(True)
    out, dens = ops.aggregate3_density(x3)
    cur, fwd, bwd = x3.detach().split(AGG_ROWS, dim=0)
    want = (cur + 0.5 * fwd + 0.5 * bwd) / 2.0
    assert torch.equal(out, want)
    xm1 = (want[:, 0] - 1.0).cpu().numpy().astype(np.float64)
    assert_ulp("aggregate3_density density", dens.detach().cpu().numpy(), np.exp(xm1), C_EXP)
    up, gd = torch.randn(AGG_ROWS, AGG_COLS, generator=g).to(_dev()), torch.randn(AGG_ROWS, generator=g).to(_dev())
    (dx,) = torch.autograd.grad([out, dens], x3, [up, gd])
    v = up.clone()
    v[:, 0] = v[:, 0] + gd * dens.detach()          # (every density here is far below the clamp e^15)
    assert float(dens.max()) < 3.0e6
    h = v / 2.0
    assert torch.equal(dx, torch.cat([h, 0.5 * h, 0.5 * h], 0))
