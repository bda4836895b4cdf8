"""Exact-arithmetic hold of fused.wgrad (emer_wgrad_segmented): the LDS-staged wgrad_seg_kernel at every tile
instantiation its dispatch reaches here, the streamed kernel as a control, and the partial-sum reduction behind both.

Every operand (dPre, col0, each segment) and the preset contents of out_w / out_b are integers, and for EVERY output
entry sum_rows |d| |x| + |preset| stays below 2^24 (asserted on the inputs, no entry left out).  All partial sums of
such an entry are integers below 2^24, so any correct kernel -- fp32 MFMA, bf16x3 MFMA (|values| <= 63 fit one bf16
term), any tile order, any order of the float atomics of the reduction -- returns the int64 product bitwise.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VMAX = 63        # |operand values|; 2048 rows x 63 x 63 = 8.1 M < 2^24
PRESET = 1000    # |preset contents| of out_w / out_b in the accumulating runs

# name -> (rows, N, segments, want_bias, col0, out_w width or None, destination columns or None)
# segments: ("rm", width) row-major | ("view", width, ld, offset) columns of a wider tensor | ("ray", width, row_div) one row per ray
#           | ("lm", L, F) level-major [L, rows, F]
CASES = {
    # K = 177 > 128: LDS-staged wgrad_seg_kernel<2,8>; per-ray operand with row_div 48, geo read through a view with ld 128
    "rgb1 336x64 K177 <2,8>": (336, 64, [("rm", 64), ("ray", 49, 48), ("view", 64, 128, 32)], True, False, None, None),
    # per-ray operand: LDS-staged <2,4>; row_div 16 puts two ray boundaries inside one 32-row tile
    "rgb0 336x64 K113 <2,4>": (336, 64, [("ray", 49, 16), ("rm", 64)], True, False, None, None),
    # K = 134 > 128: LDS-staged <1,8>; column 0 of dPre comes from col0
    "col0 129x3 K134 <1,8>": (129, 3, [("rm", 64), ("rm", 70)], True, True, None, None),
    # N = 128 > 64: LDS-staged <2,2>, two N groups; 18 row blocks of 64 rows, so the reduction runs with two splits
    "wide 1100x128 K64 <2,2>": (1100, 128, [("rm", 64)], True, False, None, None),
    # N = 48 leaves the 64 x 128 tile without its mask-free form: LDS-staged <2,4>; no bias, segments scattered into a 177-wide out_w
    "scatter 200x48 K128 <2,4>": (200, 48, [("rm", 64), ("rm", 64)], False, False, 177, [0, 113]),
    # per-ray operand: LDS-staged <1,2>; level-major segment in front of it
    "lm 160x16 K52 <1,2>": (160, 16, [("lm", 8, 4), ("ray", 20, 32)], True, False, None, None),
    # per-ray operand: LDS-staged <1,1>; 33 rows leave one row in the second tile
    "tail 33x20 K24 <1,1>": (33, 20, [("ray", 24, 11)], True, False, None, None),
    # controls on wgrad_stream_kernel (row-major operands, n <= 64, k <= 128; 64 x 128 in its mask-free vector form)
    "stream 300x64 K128": (300, 64, [("rm", 64), ("rm", 64)], True, False, None, None),
    "stream 129x3 K64": (129, 3, [("rm", 64)], True, False, None, None),
}


def _ints(rng, shape, vmax=VMAX):
    return rng.integers(-vmax, vmax + 1, size=shape).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Integer operands and the exact reference of one case, built once and shared by its runs (read-only)."""
    rows, N, segs, want_bias, col0, ow, dst = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    d = _ints(rng, (rows, N))
    c0 = _ints(rng, (rows,)) if col0 else None
    src, cols = [], []    # tensors as the kernel reads them, [rows, width] expansions as the reference reads them
    for s in segs:
        if s[0] == "rm":
            t = _ints(rng, (rows, s[1])); x = t
        elif s[0] == "view":
            t = _ints(rng, (rows, s[2])); x = t[:, s[3]:s[3] + s[1]]
        elif s[0] == "ray":
            assert rows % s[2] == 0
            t = _ints(rng, (rows // s[2], s[1])); x = np.repeat(t, s[2], 0)
        else:
            t = _ints(rng, (s[1], rows, s[2])); x = t.transpose(1, 0, 2).reshape(rows, s[1] * s[2])
        src.append(t); cols.append(x)
    x = np.concatenate(cols, 1)
    de = d.copy()
    if c0 is not None:
        assert (c0 != d[:, 0]).any()
        de[:, 0] = c0
    K = x.shape[1]
    dw, db = de.T @ x, de.sum(0)
    width = K if ow is None else ow
    starts = np.cumsum([0] + [c.shape[1] for c in cols])[:-1]
    dst = list(starts) if dst is None else dst
    scat = np.zeros((N, width), np.int64)    # dW as it lands in out_w
    for s0, c, t0 in zip(starts, cols, dst):
        scat[:, t0:t0 + c.shape[1]] = dw[:, s0:s0 + c.shape[1]]
    pre_w, pre_b = _ints(rng, (N, width), PRESET), _ints(rng, (N,), PRESET)
    # the budget, for every entry: every partial sum of the entry is an integer below 2^24
    mag = np.abs(de).T @ np.abs(x)
    assert rows <= 2048 and max(np.abs(de).max(), np.abs(x).max()) <= VMAX
    mag_w = np.zeros((N, width), np.int64)
    for s0, cc, t0 in zip(starts, cols, dst):
        mag_w[:, t0:t0 + cc.shape[1]] = mag[:, s0:s0 + cc.shape[1]]
    assert (mag_w + np.abs(pre_w) < 2 ** 24).all() and (np.abs(de).sum(0) + np.abs(pre_b) < 2 ** 24).all()
    return dict(d=d, c0=c0, src=src, K=K, dw=scat, db=db, pre_w=pre_w, pre_b=pre_b, dst=dst, starts=starts)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(DEV)


@pytest.mark.parametrize("mode", ["fresh", "accumulate"])
@pytest.mark.parametrize("name", list(CASES))
def test_wgrad_exact(hip_lib, name, mode):
    """dW, db of fused.wgrad bitwise equal to the int64 product, into fresh outputs and added onto preset out_w / out_b."""
    from emernerf_amd import fused
    rows, N, segs, want_bias, _, ow, _ = CASES[name]
    c = _case(name)
    tensors = [_t(t) for t in c["src"]]
    sg = []
    for s, t, col, dst in zip(segs, tensors, c["starts"], c["dst"]):
        col, dst = int(col), int(dst)
        if s[0] == "rm":
            sg.append(fused.seg(t, col, s[1], dst_col=dst))
        elif s[0] == "view":
            v = t[:, s[3]:s[3] + s[1]]
            assert v.stride(0) == s[2]
            sg.append(fused.seg(v, col, s[1], dst_col=dst))
        elif s[0] == "ray":
            sg.append(fused.seg(t, col, s[1], row_div=s[2], dst_col=dst))
        else:
            assert dst == col
            sg.append(fused.seg_lm(t, col))
    col0 = None if c["c0"] is None else _t(c["c0"])
    acc = mode == "accumulate"
    out_w = out_b = None
    if acc:
        out_w, out_b = _t(c["pre_w"]), (_t(c["pre_b"]) if want_bias else None)
    elif ow is not None:
        out_w = torch.zeros((N, ow), device=DEV)   # the scatter needs a destination wider than K
    dw, db = fused.wgrad(_t(c["d"]), sg, c["K"], want_bias=want_bias, col0=col0, out_w=out_w, out_b=out_b)
    fused.join_side_stream()
    torch.cuda.synchronize()
    got_w = (dw if out_w is None else out_w).cpu().numpy().astype(np.float64)
    want_w = c["dw"] + (c["pre_w"] if acc else 0)
    bad = np.argwhere(got_w != want_w)
    assert bad.size == 0, f"{name} {mode}: dW differs at {len(bad)} entries, first {bad[0]}: got {got_w[tuple(bad[0])]}, exact {want_w[tuple(bad[0])]}"
    if want_bias:
        got_b = (db if out_b is None else out_b).cpu().numpy().astype(np.float64)
        want_b = c["db"] + (c["pre_b"] if acc else 0)
        assert (got_b == want_b).all(), f"{name} {mode}: db got {got_b}, exact {want_b}"
    else:
        assert db is None
