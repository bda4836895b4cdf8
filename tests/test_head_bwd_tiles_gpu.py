"""The tile loops of the head backward kernels with register-resident weight gradients (csrc/mlp_fused.hip: rgb_bwdw16_kernel /
rgb_bwdwr_kernel behind emer_rgb_head_bwd_fused / _recompute, neck_bwdw_kernel behind emer_neck_bwd_fused) at the shapes where a loop
takes an edge: a wave with one tile, none, or exactly one more than its neighbours; a ragged last tile; a prefetch that is clamped at the
end of a wave's sequence.  The kernels prefetch one tile ahead, store one tile behind and wait with hand-placed counters, so an ordering
mistake shows as a stale or missing tile at exactly these shapes.  Reached through emernerf_amd.fused, as the training step reaches them;
bounds: tests/_bounds.py through skip3_bound / neck_bound of tests/test_fused_gpu.py, unchanged.

The per-ray sums s1 / s0 of the rgb kernels are held through what is formed from them alone: db1 / db0 (their sums over the rays; with one
ray: s1 / s0 themselves), dhray (s0 W0[:, :Kh] + s1 W1[:, H:H + Kh], per ray) and the hray blocks of dW0 / dW1."""
import pytest
import torch

from tests.test_fused_gpu import _lm_rows, neck_bound, skip3_bound

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
KH, H = 49, 64


def _rgb_run(fused, mode, hray, feats, Ws, go, S):
    fused.RGB_RECOMPUTE = mode
    hd, fd = hray.to(DEV).requires_grad_(True), feats.to(DEV).requires_grad_(True)
    wd = [w.to(DEV).requires_grad_(True) for w in Ws]
    rgb = fused.rgb_head(hd, fd, S, *wd)
    (rgb * go.to(DEV)).sum().backward()
    got = {"out": rgb.detach(), "dhray": hd.grad, "dgeo": fd.grad}
    got.update({f"{k}{i}": wd[2 * i + j].grad for i in range(3) for j, k in enumerate(("dW", "db"))})
    return got


# S = 16 / 48: one / three tiles per ray (every tile, or none, crosses a ray boundary).  1 ray: 1023 waves idle, their epilogue runs on
# zero accumulators; 1025 rays: exactly one wave takes a second ray.
@pytest.mark.parametrize("S", [16, 48])
@pytest.mark.parametrize("R", [1, 3, 1025])
def test_rgb_head_bwd_tiles(hip_lib, monkeypatch, R, S):
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_WGRAD", True)
    monkeypatch.setattr(fused, "FUSED_RGB_WGRAD", True)
    monkeypatch.setattr(fused, "RGB_RECOMPUTE", 0)
    assert fused._lib.load().emer_rgb_head_bwd_fused_workspace(R, S) > 0
    g = torch.Generator().manual_seed(1000 * R + S)
    N, K0 = R * S, KH + 64
    hray, feats = torch.randn(R, KH, generator=g), torch.randn(N, 64, generator=g)
    Ws = [torch.randn(H, K0, generator=g) / K0 ** 0.5, torch.randn(H, generator=g) * 0.1, torch.randn(H, H + K0, generator=g) / (H + K0) ** 0.5,
          torch.randn(H, generator=g) * 0.1, torch.randn(3, H, generator=g) / H ** 0.5, torch.randn(3, generator=g) * 0.1]
    go = torch.randn(N, 3, generator=g)
    stored = _rgb_run(fused, 0, hray, feats, Ws, go, S)        # emer_rgb_head_bwd_fused
    recomputed = _rgb_run(fused, 1, hray, feats, Ws, go, S)    # emer_rgb_head_bwd_recompute, a1 and a2 recomputed
    inp = torch.cat([hray.double().repeat_interleave(S, dim=0), feats.double()], -1)
    skip3_bound(f"rgb_head tiles R{R} S{S}", inp, Ws, go.double(), True, stored, per_ray=S, kh=KH)
    # the two kernels run the same stages behind their inputs: equal to the bit.  The weight and bias gradients are compared where their
    # final reduction meets in no float atomic (at most 16 rays: one workgroup range, as tests/test_fused_gpu.py documents)
    for k in stored:
        if k in ("out", "dhray", "dgeo") or R <= 16:
            assert torch.equal(stored[k], recomputed[k]), f"R{R} S{S} {k}: fused and recompute differ"


# L16 / F2: neck_bwdw_kernel<2, 2, 1>.  n = 1; 21: one full and one ragged tile; 16 * 2048 + 5: every wave of a full grid gets one tile and
# the last is ragged; 48: most waves have an empty range.
@pytest.mark.parametrize("N", [1, 21, 16 * 2048 + 5, 16 * 3])
def test_neck_bwd_tiles(hip_lib, monkeypatch, N):
    from emernerf_amd import fused
    monkeypatch.setattr(fused, "FUSED_WGRAD", True)
    L, Fe, NG = 16, 2, 64
    K0 = L * Fe
    assert fused._lib.load().emer_neck_bwd_fused_workspace(L, Fe, N, NG) > 0
    g = torch.Generator().manual_seed(77 + N)
    NP = N + 19   # rows past n: the kernel is given n rows of a larger tensor and must leave the others alone
    enc_all = torch.randn(L, NP, Fe, generator=g)
    W0, b0 = torch.randn(H, K0, generator=g) / K0 ** 0.5, torch.randn(H, generator=g) * 0.1
    W1, b1 = torch.randn(NG, H, generator=g) / H ** 0.5, torch.randn(NG, generator=g) * 0.1
    gg, gd = torch.randn(N, 64, generator=g), torch.randn(N, generator=g)
    enc = enc_all[:, :N].contiguous()
    t = [v.to(DEV).requires_grad_(True) for v in (enc, W0, b0, W1, b1)]
    geo, sem, dens = fused.neck(*t)
    assert sem is None
    ((geo * gg.to(DEV)).sum() + (dens * gd.to(DEV)).sum()).backward()
    x = enc.double().permute(1, 0, 2).reshape(N, K0)
    neck_bound(f"neck tiles N{N}", x, W0, b0, W1, b1, gg.double(), gd.double(),
               {"feats": geo, "density": dens, "dx": _lm_rows(t[0].grad, N), "dW0": t[1].grad, "db0": t[2].grad, "dW1": t[3].grad, "db1": t[4].grad})
    # Rows past n keep a sentinel written before the call.  denc is level-major [L][n][F] and dense: a lane of the ragged tile that stored
    # its row >= n would hit the first rows of the NEXT level (shown by the comparison with the autograd path's denc) or, in the last
    # level, the memory behind the tensor: the entry point is called on a buffer with 19 sentinel rows behind it.
    from emernerf_amd import _lib
    p = lambda v: v.data_ptr()   # noqa: E731
    d0, ddens = gg.to(DEV), gd.to(DEV)
    encd, w0d, b0d, w1d = (v.detach() for v in t[:4])
    ws = torch.empty(int(_lib.load().emer_neck_bwd_fused_workspace(L, Fe, N, NG)), device=DEV)
    denc = torch.full((L * N * Fe + 19 * Fe,), -3.25, device=DEV)   # n rows of L levels, and 19 rows more behind the last level
    dw0, db0, dw1, db1 = (torch.zeros(s, device=DEV) for s in ((H, K0), (H,), (NG, H), (NG,)))
    _lib.call("emer_neck_bwd_fused", p(d0), None, p(ddens), p(dens.detach()), p(encd), L, Fe, N, p(w0d), p(b0d), p(w1d), NG, p(denc), p(ws),
              p(dw0), K0, p(db0), p(dw1), 64, p(db1), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(denc[:L * N * Fe].view(L, N, Fe), t[0].grad), "denc of the direct call differs from the autograd path's"
    assert bool((denc[L * N * Fe:] == -3.25).all()), "rows past n of denc were written"
