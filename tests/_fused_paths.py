"""One case per row of the path table of emernerf_amd/fused.py (its module docstring): the head, the flags, the smallest shape
that still has two tiles or two rays, and the path its Function must record (test helper, not a test module).

The cases use only the public functions and the five module flags, so the same table runs against any checkout of the package:
tests/test_fused_paths_gpu.py pins the path and the library calls of each case, tools/head_digests.py digests their results and
lists their device kernels.  emernerf_amd is imported when a case is built, never at import of this module."""
import contextlib
import zlib

import torch

from tests._chain_probe import BASE_CASES, RGB_CASES, SEQ_CHAIN

DEFAULT_FLAGS = dict(FUSED_WGRAD=True, FUSED_RMLP_WGRAD=True, FUSED_RMLP_WIDE=True, FUSED_RGB_WGRAD=True, RGB_RECOMPUTE=0)
BACKWARD = "-- backward --"   # the marker run_case puts between the two passes into a recorded list of names


@contextlib.contextmanager
def flags(**kw):
    """The five flags of emernerf_amd.fused set to their defaults overridden by kw, restored on exit."""
    from emernerf_amd import fused
    want = dict(DEFAULT_FLAGS, **kw)
    prev = {k: getattr(fused, k) for k in want}
    for k, v in want.items():
        setattr(fused, k, v)
    try:
        yield
    finally:
        for k, v in prev.items():
            setattr(fused, k, v)


def _leaves(dev, seed, *specs):
    """Seeded CPU draws moved to the device as leaves: specs of (shape, scale)."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(*shape, generator=g) * k).to(dev).requires_grad_(True) for shape, k in specs]


def _mlp_specs(dims):
    ws = [((dims[i + 1], dims[i]), dims[i] ** -0.5) for i in range(len(dims) - 1)]
    bs = [((dims[i + 1],), 0.1) for i in range(len(dims) - 1)]
    return ws, bs


def _skip_specs(H, K0, C):
    return [((H, K0), K0 ** -0.5), ((H,), 0.1), ((H, H + K0), (H + K0) ** -0.5), ((H,), 0.1), ((C, H), H ** -0.5), ((C,), 0.1)]


def rgb(R, S, Kh, NG=64, H=64, C=3, ld=None):
    """-> (build(dev) -> (call, leaves), rows that meet in one weight-gradient sum)."""
    def build(dev):
        from emernerf_amd import fused
        t = _leaves(dev, R * S + Kh, ((R, Kh), 1.0), ((R * S, ld or NG), 1.0), *_skip_specs(H, Kh + NG, C))
        return (lambda: [fused.rgb_head(t[0], t[1][:, :NG], S, *t[2:])]), t
    return build, R


def neck(L, F, n_out, N):
    def build(dev):
        from emernerf_amd import fused
        t = _leaves(dev, 7 * L + n_out + N, ((L, N, F), 1.0), ((64, L * F), (L * F) ** -0.5), ((64,), 0.1), ((n_out, 64), 0.125), ((n_out,), 0.1))
        return (lambda: list(fused.neck(*t))), t
    return build, N


def density(L, F, N, H=64):
    def build(dev):
        from emernerf_amd import fused
        t = _leaves(dev, 5 * L + F + N, ((L, N, F), 1.0), ((H, L * F), (L * F) ** -0.5), ((H,), 0.1), ((1, H), H ** -0.5), ((1,), 0.1))
        return (lambda: [fused.density_mlp(*t)]), t
    return build, N


def base(L, F, H, NG, N):
    def build(dev):
        from emernerf_amd import fused
        t = _leaves(dev, 3 * L + H + N, ((L, N, F), 1.0), ((H, L * F), (L * F) ** -0.5), ((H,), 0.1), ((NG, H), H ** -0.5), ((NG,), 0.1))
        return (lambda: list(fused.base_mlp(*t))), t
    return build, N


def skip(N, K0, H=64, C=3):
    def build(dev):
        from emernerf_amd import fused
        t = _leaves(dev, N + K0, ((N, K0), 1.0), *_skip_specs(H, K0, C))
        return (lambda: [fused.skip_mlp3(*t)]), t
    return build, N


def seq(dims, N, lm=None):
    """Row-major input [N, dims[0]], or with lm = (L, F) the level-major [L, N, F] (dims[0] = L F)."""
    def build(dev):
        from emernerf_amd import fused
        ws, bs = _mlp_specs(dims)
        n = len(ws)
        t = _leaves(dev, sum(dims) + N, (((N, dims[0]) if lm is None else (lm[0], N, lm[1])), 1.0), *ws, *bs)
        fn = fused.seq_mlp if lm is None else fused.seq_mlp_lm
        return (lambda: [fn(t[0], t[1:1 + n], t[1 + n:])]), t
    return build, N


_H, _Kh, _NG, _C, _R, _S = RGB_CASES[0]
_bL, _bF, _bH, _bNG, _bN = BASE_CASES[0]
# id: (head, the path its Function records, flags other than the defaults, (build, rows))
CASES = {
    "rgb fused": ("rgb_head", "fused", {}, rgb(2, 16, 49)),
    "rgb recompute_a1a2": ("rgb_head", "recompute_a1a2", dict(RGB_RECOMPUTE=1), rgb(2, 16, 49)),
    "rgb recompute_a2": ("rgb_head", "recompute_a2", dict(RGB_RECOMPUTE=2), rgb(2, 16, 49)),
    "rgb w2_in_kernel": ("rgb_head", "w2_in_kernel", dict(FUSED_RGB_WGRAD=False), rgb(2, 16, 49)),
    "rgb streamed": ("rgb_head", "streamed", dict(FUSED_WGRAD=False, FUSED_RGB_WGRAD=False), rgb(2, 16, 49)),
    "rgb chain": ("rgb_head", "chain", {}, rgb(_R, _S, _Kh, _NG, _H, _C)),
    "neck 4x2 64 fused": ("neck", "fused", {}, neck(4, 2, 64, 33)),
    "neck 4x2 64 streamed": ("neck", "streamed", dict(FUSED_WGRAD=False), neck(4, 2, 64, 33)),
    "neck 10x4 128 fused": ("neck", "fused", {}, neck(10, 4, 128, 33)),
    "neck 10x4 128 streamed": ("neck", "streamed", dict(FUSED_WGRAD=False), neck(10, 4, 128, 33)),
    "density 8x1 fused": ("density_mlp", "fused", {}, density(8, 1, 17)),
    "density 8x1 neck_streamed": ("density_mlp", "neck_streamed", dict(FUSED_WGRAD=False), density(8, 1, 17)),
    "density 12x2 neck_streamed": ("density_mlp", "neck_streamed", {}, density(12, 2, 17)),
    "density chain": ("density_mlp", "chain", {}, density(_bL, _bF, 17, H=_bH)),
    "base chain": ("base_mlp", "chain", {}, base(_bL, _bF, _bH, _bNG, _bN)),
    "skip ray": ("skip_mlp3", "ray", {}, skip(33, 43)),
    "skip ray_streamed": ("skip_mlp3", "ray_streamed", {}, skip(65537, 43)),
    "skip chain": ("skip_mlp3", "chain", {}, skip(33, 70)),
    "seq 40-64-64-6 fused": ("seq_mlp", "fused", {}, seq((40, 64, 64, 6), 17)),
    "seq 40-64-64-6 streamed": ("seq_mlp", "streamed", dict(FUSED_RMLP_WGRAD=False), seq((40, 64, 64, 6), 17)),
    "seq_lm 10x4 fused": ("seq_mlp_lm", "fused", {}, seq((40, 64, 64, 6), 17, lm=(10, 4))),
    "seq_lm 10x4 streamed": ("seq_mlp_lm", "streamed", dict(FUSED_WGRAD=False), seq((40, 64, 64, 6), 17, lm=(10, 4))),
    "seq 64-64-64-64 fused": ("seq_mlp", "fused", {}, seq((64, 64, 64, 64), 17)),
    "seq 64-64-64-64 streamed": ("seq_mlp", "streamed", dict(FUSED_RMLP_WIDE=False), seq((64, 64, 64, 64), 17)),
    "seq chain": ("seq_mlp", "chain", {}, seq(SEQ_CHAIN[0], 17)),
}


def run_case(case_id, dev, names=None, before_backward=None):
    """One forward and one backward of the case under its flags -> (outputs, leaves with .grad).  names: a list that a recorder
    wrapped around emernerf_amd._lib.call appends to; BACKWARD is put between the passes.  before_backward: called after the
    forward (the test of a flag changed between the passes)."""
    _, _, fl, (build, _) = CASES[case_id]
    with flags(**fl):
        call, leaves = build(dev)
        outs = [o for o in call() if o is not None]
        g = torch.Generator().manual_seed(zlib.crc32(case_id.encode()))
        gos = [torch.randn(*o.shape, generator=g).to(dev) for o in outs]
        if names is not None:
            names.append(BACKWARD)
        if before_backward is not None:
            before_backward()
        torch.autograd.backward(outs, gos)
    return outs, leaves
