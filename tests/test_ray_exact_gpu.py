"""The per-ray head kernels of csrc/rayinputs.hip held bit for bit to fp64 on exact probes (tests/_ray_probe.py), each case
once through its stand-alone entry point ("alone") and once as a member of an emer_ray_jobs launch ("job", never the only
member nor the first, so the member's own workgroup numbering is exercised).  tests/test_ray_jobs_gpu.py compares the two
sides with each other; this module is what holds the trusted side itself.

Every case checks the < 2^24 units budget per entry on its inputs (the builders and ``assert_exact``), prints the cover of
every output, hands the kernel outputs filled with a NaN sentinel and requires padding columns, untouched columns, a guard row
behind the last row and table rows no ray uses to come back with the bits they had.  The sin columns of the direction rows are held to ``E_SINF`` ulps of the fp64
sin of the fp32 argument the kernel forms (tests/_bounds.py: measured on the device).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _ray_probe as P
from tests._bounds import E_SINF

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VIA = ["alone", "job"]


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _p(t):
    return None if t is None else t.data_ptr()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _act(b):
    from emernerf_amd._lib import ACT_NONE, ACT_SIGMOID
    return ACT_SIGMOID if b["act"] else ACT_NONE


def _print_covers(what, report):
    print(f"\n[cover] {what}: " + ", ".join(f"{k.split(' ')[-1]} {v:.3f}" for k, v in report.items()))


_build_pre = functools.lru_cache(maxsize=None)(P.build_pre)
_build_head = functools.lru_cache(maxsize=None)(P.build_head)
_build_wgrad = functools.lru_cache(maxsize=None)(P.build_wgrad)
_build_embed = functools.lru_cache(maxsize=None)(P.build_embed)
_build_chain = functools.lru_cache(maxsize=None)(P.build_chain)


# ------------------------------------------------------------------------------------------------------ ray_pre_fwd / bwd
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("Kh,H,R,null", P.PRE_SHAPES)
def test_ray_pre_exact(hip_lib, Kh, H, R, null, via):
    """rb = [W0[:, :Kh] h + ba | W1[:, H:H+Kh] h + bb] and d h = s0 W0[:, :Kh] + s1 W1[:, H:H+Kh] on weight blocks of wider
    matrices, ld_h > Kh, ld_rb > 2H, ld_s > H, ld_dh > Kh; ba / bb null once each."""
    from emernerf_amd import _lib, ray_jobs as rj
    b = _build_pre(Kh, H, R, null)
    W0, W1, hw, s0w, s1w, ba, bb = (T(b[k]) for k in ("W0", "W1", "h_wide", "s0_wide", "s1_wide", "ba", "bb"))
    rb, dh = T(P.sentinel((R + 1, 2 * H + 3))), T(P.sentinel((R + 1, Kh + 3)))   # (one guard row behind the R the kernel is told)
    h, s0, s1, wb = hw[:, :Kh], s0w[:, :H], s1w[:, :H], W1[:, H:]
    if via == "alone":
        _lib.call("emer_ray_pre_fwd", h.data_ptr(), hw.stride(0), R, Kh, H, W0.data_ptr(), W0.stride(0), _p(ba), wb.data_ptr(), W1.stride(0), _p(bb),
                  rb.data_ptr(), rb.stride(0), _st())
        _lib.call("emer_ray_pre_bwd", s0.data_ptr(), s1.data_ptr(), s0w.stride(0), R, Kh, H, W0.data_ptr(), W0.stride(0), wb.data_ptr(), W1.stride(0),
                  dh.data_ptr(), dh.stride(0), _st())
    else:
        rj.launch([rj.job(rj.PRE_BWD, rj.pre_bwd_args(s0, s1, Kh, W0, W1, dh)), rj.job(rj.PRE_FWD, rj.pre_fwd_args(h, W0, ba, W1, bb, rb))], rb)
    torch.cuda.synchronize()
    report = {}
    P.check_pre(b, N(rb), N(dh), f"{via} Kh={Kh} H={H} R={R}", report)
    _print_covers(f"ray_pre {via} Kh={Kh} H={H} R={R}", report)


# ----------------------------------------------------------------------------------------------------- ray_head_fwd / bwd
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("dense", P.HEAD_DENSE)
@pytest.mark.parametrize("C,act,R,no_b2", P.HEAD_CASES)
def test_ray_head_exact(hip_lib, C, act, R, no_b2, dense, via):
    """The sky head after ray_pre_fwd, forward and data gradients: a1, a2, dpre2, dpre1, dpre0 bit for bit with one layer dense
    per probe; out bit for bit without an activation (layer 2 dense: cover 1.0), within C_SIG u of the sigmoid of the exact
    pre-activation with one.  ld_rb = 132, ld_w1 = 69; the backward's masks carry +0, -0 and 2^-126."""
    from emernerf_amd import _lib, ray_jobs as rj
    b = _build_head(C, act, R, dense, no_b2)
    rbw, W1, W2, b2, dout, y, a1m, a2m = (T(b[k]) for k in ("rb_wide", "W1", "W2", "b2", "dout", "y", "a1m", "a2m"))
    a1, a2, out = (T(P.sentinel((R + 1, w))) for w in (64, 64, C))   # (one guard row each)
    d2, d1, d0 = (T(P.sentinel((R + 1, w))) for w in (C, 64, 64))
    A = _act(b)
    if via == "alone":
        _lib.call("emer_ray_head_fwd", rbw.data_ptr(), rbw.stride(0), R, W1.data_ptr(), W1.stride(0), W2.data_ptr(), _p(b2), C, A,
                  a1.data_ptr(), a2.data_ptr(), out.data_ptr(), _st())
        _lib.call("emer_ray_head_bwd", dout.data_ptr(), y.data_ptr(), a1m.data_ptr(), a2m.data_ptr(), R, W1.data_ptr(), W1.stride(0), W2.data_ptr(), C, A,
                  d2.data_ptr(), d1.data_ptr(), d0.data_ptr(), _st())
    else:
        rj.launch([rj.job(rj.HEAD_BWD, rj.head_bwd_args(dout, y, a1m, a2m, W1, W2, A, d2, d1, d0)),
                   rj.job(rj.HEAD_FWD, rj.head_fwd_args(rbw, W1, W2, b2, A, a1, a2, out))], rbw)
    torch.cuda.synchronize()
    report = {}
    what = f"{via} C={C} act={act} R={R} dense={dense}"
    P.check_head_fwd(b, N(a1), N(a2), N(out), what, report)
    P.check_head_bwd(b, N(d2), N(d1), N(d0), what, report)
    _print_covers(f"ray_head {what}", report)


# --------------------------------------------------------------------------------------------------------------- ray_wgrad
@pytest.mark.parametrize("preload", [0, 1])
@pytest.mark.parametrize("M", P.WG_M)
def test_ray_wgrad_exact(hip_lib, M, preload):
    """Twelve jobs (P.WG_JOBS) as a full launch of EMER_RAY_WGRAD_MAX_JOBS and a launch of four, through emer_ray_wgrad and as
    members of emer_ray_jobs launches: every dW / db entry bit for bit onto zeroed and preloaded targets, also beyond one
    256-row chunk (several atomics per entry); ld_dy > n, ld_x > width, dst_col > 0, the columns between the blocks untouched."""
    from emernerf_amd import fused, ray_jobs as rj
    jobs = _build_wgrad(M, preload)
    assert P.WG_MAX_JOBS == rj.MAX_JOBS == 8
    dys = [T(j["dy_wide"]) for j in jobs]
    xs = [[T(x) for x in j["x_wide"]] for j in jobs]
    report = {}
    for via in VIA:
        tgt = [(T(np.concatenate([j["dw0"], P.sentinel((1, j["dw0"].shape[1]))], 0)), T(j["db0"])) for j in jobs]   # (a guard row behind dw)
        tup = [(dys[i][:M, :j["n"]], [(xs[i][k][:M, :w], w, j["dst"][k]) for k, w in enumerate(j["widths"])], tgt[i][0][:j["n"]], tgt[i][1]) for i, j in enumerate(jobs)]
        for part in (tup[:P.WG_MAX_JOBS], tup[P.WG_MAX_JOBS:]):
            if via == "alone":
                fused.ray_wgrad(part, dys[0])
            else:
                rj.launch([rj.wgrad_job(*t) for t in part], dys[0])
        torch.cuda.synchronize()
        for i, j in enumerate(jobs):
            P.check_wgrad(j, N(tgt[i][0]), None if tgt[i][1] is None else N(tgt[i][1]), f"{via} M={M} preload={preload} job {i}", report)
    print(f"\n[cover] ray_wgrad M={M} preload={preload}: {len(report)} outputs, min cover {min(report.values()):.3f}")


# -------------------------------------------------------------------------------------------------------------- embed_grad
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("R,n_emb,E,which", P.EMB_CASES)
def test_embed_grad_exact(hip_lib, R, n_emb, E, which, via):
    """dw[idx[r]] += g_a[r] + g_b[r] onto a preloaded table, strided indices, g_a or g_b null, negative and too large indices
    contributing nowhere, unused rows untouched; two runs (two launches / two members of one launch) identical."""
    from emernerf_amd import _lib, ray_jobs as rj
    b = _build_embed(R, n_emb, E, which)
    idxw, gaw, gbw = T(b["idx_wide"]), T(b["ga_wide"]), T(b["gb_wide"])
    idx = idxw[:, 1]
    ga = None if gaw is None else gaw[:, P.EMB_P:]
    gb = None if gbw is None else gbw[:, P.EMB_P:]
    lda, ldb = (0 if gaw is None else gaw.stride(0)), (0 if gbw is None else gbw.stride(0))
    runs = [T(b["dw0"]), T(b["dw0"])]
    if via == "alone":
        for dw in runs:
            _lib.call("emer_embed_grad", _p(ga), lda, _p(gb), ldb, idx.data_ptr(), idx.stride(0), R, n_emb, E, dw.data_ptr(), _st())
    else:
        rj.launch([rj.job(rj.EMBED_GRAD, rj.embed_grad_args(ga, lda, gb, ldb, idx, n_emb, E, dw)) for dw in runs], idxw)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    report = {}
    P.check_embed(b, N(runs[1]), f"{via} R={R} n_emb={n_emb} E={E}", report)
    _print_covers(f"embed_grad {via} R={R} n_emb={n_emb} E={E} g={which}", report)


# ------------------------------------------------------------------------------------------------------------ forward chain
@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("R", P.CHAIN_R)
def test_forward_chain_exact(hip_lib, R, via):
    """inputs -> pre_fwd -> head_fwd with identity direction rows (max_deg = 0) on grid operands: rows, rb, a1, a2 bit for bit,
    out within C_SIG u -- as three launches, and as one three-stage chain job next to an inputs job for the rgb rows."""
    from emernerf_amd import _lib, ray_jobs as rj
    from emernerf_amd._lib import ACT_SIGMOID
    b = _build_chain(R)
    Kh, E = b["Kh"], b["E"]
    dirs, emb, idx, W0, b0, W1, b1, W2, b2 = (T(b[k]) for k in ("dirs", "emb", "idx", "W0", "b0", "W1", "b1", "W2", "b2"))
    x_rgb, x_sky = T(P.sentinel((R + 1, Kh))), T(P.sentinel((R + 1, Kh)))   # (one guard row behind every output)
    rb, a1, a2, out = (T(P.sentinel((R + 1, w))) for w in (128, 64, 64, 3))
    if via == "alone":
        _lib.call("emer_ray_inputs_fwd", dirs.data_ptr(), 3, idx.data_ptr(), 1, emb.data_ptr(), b["n_emb"], E, 0, R, x_rgb.data_ptr(), Kh, x_sky.data_ptr(), Kh, _st())
        _lib.call("emer_ray_pre_fwd", x_sky.data_ptr(), Kh, R, Kh, 64, W0.data_ptr(), W0.stride(0), b0.data_ptr(), W1[:, 64:].data_ptr(), W1.stride(0),
                  b1.data_ptr(), rb.data_ptr(), 128, _st())
        _lib.call("emer_ray_head_fwd", rb.data_ptr(), 128, R, W1.data_ptr(), W1.stride(0), W2.data_ptr(), b2.data_ptr(), 3, ACT_SIGMOID,
                  a1.data_ptr(), a2.data_ptr(), out.data_ptr(), _st())
    else:
        rj.launch([rj.job(rj.INPUTS, rj.inputs_args(dirs, idx, emb, 0, x_rgb, None)),
                   rj.fwd_chain_job(rj.inputs_args(dirs, idx, emb, 0, None, x_sky), rj.pre_fwd_args(x_sky[:R], W0, b0, W1, b1, rb),
                                    rj.head_fwd_args(rb[:R], W1, W2, b2, ACT_SIGMOID, a1, a2, out))], dirs)
    torch.cuda.synchronize()
    report = {}
    P.check_chain(b, N(x_sky), N(rb), N(a1), N(a2), N(out), f"{via} chain R={R}", report)
    P.assert_exact(f"{via} chain R={R} rgb rows", P.live_rows(N(x_rgb), R, "rgb rows"), b["x_rgb"], None, 1.0, report)
    _print_covers(f"forward chain {via} R={R}", report)


# ------------------------------------------------------------------------------------------- sin columns of the direction rows
@pytest.mark.parametrize("n", P.DIR_N)
@pytest.mark.parametrize("remap", [False, True])
@pytest.mark.parametrize("max_deg", P.DIR_DEGS)
def test_dir_encode_sin_columns(hip_lib, max_deg, remap, n):
    from emernerf_amd import ops
    d, grid = P.build_dirs(n)
    out = ops.dir_encode(T(d), max_deg, remap=remap)
    torch.cuda.synchronize()
    P.check_dir_rows(N(out), d, grid, max_deg, remap, E_SINF, f"dir_encode deg={max_deg} remap={remap} n={n}")


@pytest.mark.parametrize("via", VIA)
@pytest.mark.parametrize("n", P.DIR_N)
@pytest.mark.parametrize("max_deg", P.DIR_DEGS)
def test_ray_inputs_rows(hip_lib, max_deg, n, via):
    """[PE(remapped d) | emb[idx]] and [PE(raw d) | emb[idx]] into rows of wider tensors: PE columns as for emer_dir_encode,
    embedding columns bit for bit, padding columns untouched."""
    from emernerf_amd import _lib, ray_jobs as rj
    d, grid = P.build_dirs(n)
    rng = np.random.default_rng(n + max_deg)
    E, n_emb = 5, 3
    emb = rng.standard_normal((n_emb, E)).astype(np.float32)
    idxw = rng.integers(0, n_emb, size=(n, 2)).astype(np.int64)
    W = P.dir_width(max_deg) + E
    dirs, embd, idxd = T(d), T(emb), T(idxw)
    idx = idxd[:, 1]
    o_rgb, o_sky = T(P.sentinel((n, W + 2))), T(P.sentinel((n, W + 2)))
    if via == "alone":
        _lib.call("emer_ray_inputs_fwd", dirs.data_ptr(), 3, idx.data_ptr(), idx.stride(0), embd.data_ptr(), n_emb, E, max_deg, n,
                  o_rgb.data_ptr(), o_rgb.stride(0), o_sky.data_ptr(), o_sky.stride(0), _st())
    else:
        rj.launch([rj.job(rj.INPUTS, rj.inputs_args(dirs, idx, embd, max_deg, None, o_sky)), rj.job(rj.INPUTS, rj.inputs_args(dirs, idx, embd, max_deg, o_rgb, None))], dirs)
    torch.cuda.synchronize()
    for name, o, remap in (("rgb", N(o_rgb), True), ("sky", N(o_sky), False)):
        what = f"ray_inputs {via} {name} deg={max_deg} n={n}"
        assert P.is_sentinel(o[:, W:]), f"{what}: padding columns were written"
        P.check_dir_rows(o[:, :W - E], d, grid, max_deg, remap, E_SINF, what)
        assert np.array_equal(o[:, W - E:W].view(np.uint32), emb[idxw[:, 1]].view(np.uint32)), f"{what}: embedding columns"


def test_device_sinf_error_is_inside_E_SINF(hip_lib):
    """A smaller run of the sweep E_SINF was measured on (P.sinf_sweep: uniform in [-1026, 1026] and [-2, 2], log-spaced
    magnitudes, the neighbourhoods of every zero crossing and extremum up to 326 pi, the 2^-10 grid times 2^k, x 2^k of uniform
    x), through emer_dir_encode (remap off, max_deg = 1: sinf of x, 2 x, x + pi/2, 2 x + pi/2)."""
    from emernerf_amd import ops
    a = P.sinf_sweep(17)
    out = N(ops.dir_encode(T(a.reshape(-1, 3)), 1, remap=False))
    worst = P.sinf_sweep_error(a, out)
    print(f"\n[sinf] device sweep of {a.size * 4} arguments: worst {worst['max_ulp']:.3f} ulp at {worst['at']!r} (E_SINF {E_SINF})")
    assert worst["max_ulp"] <= E_SINF
