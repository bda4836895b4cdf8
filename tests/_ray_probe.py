"""Exact probes, fp64 references and fp32 operation-order models for the per-ray head kernels of csrc/rayinputs.hip (test
helper, not a test module): emer_ray_pre_fwd / bwd, emer_ray_head_fwd / bwd, emer_ray_wgrad, emer_embed_grad, the direction
rows of emer_dir_encode / emer_ray_inputs_fwd.

These kernels are fp32 fmaf chains, v_mfma_f32_16x16x4_f32 and float atomics, with no bf16 split.  The argument is the one of
tests/_head_probe.py with a single plane: operands on fixed-point grids, sum_k |a| |b| + |bias| + |preloaded target| < 2^24
grid units for an output entry (checked per entry on the inputs: ``BUDGET``), so every partial sum of that entry -- in any
order, through any number of atomics -- is exactly representable in fp32 and a correct kernel returns the fp64 result bit
for bit.  A builder returns the operands as the kernel reads them (views of wider arrays: every row stride exceeds the
width), the fp64 reference and the per-entry units; ``check_*`` holds a set of outputs to them and is what the GPU tests
(tests/test_ray_exact_gpu.py) and the CPU tests of the numpy models (tests/test_ray_bounds_cpu.py) both call.  Outputs are
handed to the kernel filled with ``SENTINEL`` (a NaN with a payload no arithmetic produces); padding columns and untouched
columns must come back with exactly those bits.

``model_*`` restate each stage in fp32 in the kernel's own operation order (``mut`` selects one of ``MUTANTS``: one-line slips
of the kind these kernels invite).  Unmutated they pass every probe; each mutant fails the probe family named for it.
"""
import numpy as np

from tests._bounds import C_SIG
from tests._head_probe import BUDGET, abs_units, assert_exact, assert_ulp, grid_of, grid_values, on_grid, signed_perm, sparse_rows

F32, F64 = np.float32, np.float64
SENTINEL = 0x7FC0DEAD
TILE = 32          # rows per workgroup of the row-local stages


def sentinel(shape) -> np.ndarray:
    return np.full(shape, SENTINEL, np.uint32).view(F32)


def is_sentinel(x) -> bool:
    return bool((np.ascontiguousarray(x, F32).view(np.uint32) == SENTINEL).all())


def _a(x):
    return np.asarray(x, F64)


def live_rows(x, rows: int, what: str):
    """x[:rows], after checking that any guard rows behind them (outputs may be handed over longer than the row count the
    kernel is told) still hold the sentinel."""
    x = np.asarray(x, F32)
    assert is_sentinel(x[rows:]), f"{what}: rows past the end were written"
    return x[:rows]


def _units(a, b, extra, q: int):
    """(|b| |a|^T + |extra|) in units of 2^-q; a [n, k], b [rows, k], extra broadcastable to [rows, n]; all on their grids."""
    assert grid_of(a) + grid_of(b) <= q, "operands off their grids"
    s = abs_units(a, b, None, q)
    if extra is not None:
        assert on_grid(extra, q), "addend off the product grid"
        s = s + np.abs(_a(extra)) * 2.0 ** q
    return s


def fma_chain(acc, x, w):
    """acc[r, n] = fmaf(x[r, k], w[n, k], acc[r, n]) for k = 0, 1, ...: one rounding per step (the product of two fp32 values
    is exact in fp64; the double rounding of the sum is immaterial next to the probes, which are exact)."""
    acc = np.array(acc, F32)
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    for k in range(x.shape[1]):
        acc = (acc.astype(F64) + x[:, k][:, None].astype(F64) * w[:, k][None, :]).astype(F32)
    return acc


def _swap_tail_rows(v, R):
    """Mutant: rows 2q and 2q + 1 exchanged in a partial last tile (a row whose partner lies past the end gets zeros)."""
    v = np.array(v)
    t0 = (R // TILE) * TILE
    if t0 == R:
        return v
    out = v.copy()
    for r in range(t0, R):
        out[r] = v[r ^ 1] if (r ^ 1) < R else 0.0
    return out


# ===================================================================================================== ray_pre_fwd / bwd
# (Kh, H, R, null bias): every value of the issue's sets once, the corners Kh = H = 64 and Kh = H = 1
PRE_SHAPES = [(1, 1, 1, ""), (2, 16, 31, "ba"), (7, 63, 32, "bb"), (33, 64, 33, ""), (49, 1, 45, ""), (63, 16, 1, ""), (64, 64, 45, "")]


def build_pre(Kh, H, R, null="", seed=0):
    """8-bit x 8-bit operands on 2^-8, biases on the product grid 2^-16: <= 64 (fwd) / 128 (bwd) products of < 2^16 units."""
    rng = np.random.default_rng(1000 * Kh + 10 * H + R + seed)
    b = dict(Kh=Kh, H=H, R=R)
    b["W0"] = grid_values(rng, (H, Kh + 5), 8, 8)
    b["W1"] = grid_values(rng, (H, H + Kh + 3), 8, 8)
    b["h_wide"] = grid_values(rng, (R, Kh + 2), 8, 8, nonzero=False)
    b["ba"] = None if null == "ba" else grid_values(rng, (H,), 20, 16, nonzero=False)
    b["bb"] = None if null == "bb" else grid_values(rng, (H,), 20, 16, nonzero=False)
    b["s0_wide"], b["s1_wide"] = grid_values(rng, (2, R, H + 2), 8, 8, nonzero=False)
    wa, wb, h = b["W0"][:, :Kh], b["W1"][:, H:H + Kh], b["h_wide"][:, :Kh]
    s0, s1 = b["s0_wide"][:, :H], b["s1_wide"][:, :H]
    z = np.zeros(H)
    b["rb"] = np.concatenate([_a(h) @ _a(wa).T + (z if b["ba"] is None else _a(b["ba"])), _a(h) @ _a(wb).T + (z if b["bb"] is None else _a(b["bb"]))], 1)
    b["u_rb"] = np.concatenate([_units(wa, h, b["ba"], 16), _units(wb, h, b["bb"], 16)], 1)
    b["dh"] = _a(s0) @ _a(wa) + _a(s1) @ _a(wb)
    b["u_dh"] = _units(np.concatenate([wa, wb], 0).T, np.concatenate([s0, s1], 1), None, 16)
    return b


def check_pre(b, rb_wide, dh_wide, what, report=None):
    """rb_wide [R, 2H + 3], dh_wide [R, Kh + 3] as the kernels left them (either may be None)."""
    H, Kh = b["H"], b["Kh"]
    rb_wide = None if rb_wide is None else live_rows(rb_wide, b["R"], f"{what} rb")
    dh_wide = None if dh_wide is None else live_rows(dh_wide, b["R"], f"{what} dh")
    if rb_wide is not None:
        assert is_sentinel(rb_wide[:, 2 * H:]), f"{what}: rb padding columns were written"
        assert_exact(f"{what} rb", rb_wide[:, :2 * H], b["rb"], b["u_rb"], 1.0, report)
    if dh_wide is not None:
        assert is_sentinel(dh_wide[:, Kh:]), f"{what}: dh padding columns were written"
        assert_exact(f"{what} dh", dh_wide[:, :Kh], b["dh"], b["u_dh"], 1.0, report)


def model_pre_fwd(h, wa, ba, wb, bb, mut=""):
    """rb [R, 2H]: per output column an fmaf chain over k = 0 .. Kh-1 that starts from the bias."""
    R, H = h.shape[0], wa.shape[0]
    za = np.zeros(H, F32) if ba is None else np.asarray(ba, F32)
    zb = np.zeros(H, F32) if bb is None else np.asarray(bb, F32)
    if mut == "pre_bias_b_from_a":
        zb = za
    lo = fma_chain(np.broadcast_to(za, (R, H)), h, wa)
    hi = fma_chain(np.broadcast_to(zb, (R, H)), h, wb)
    return np.concatenate([hi, lo] if mut == "pre_halves_swapped" else [lo, hi], 1)


def model_pre_bwd(s0, s1, wa, wb, mut=""):
    """dh [R, Kh]: an fmaf chain over the 2H columns of [s0 | s1] from zero."""
    R = s0.shape[0]
    s = np.concatenate([s0, np.zeros_like(s1) if mut == "pre_bwd_s1_dropped" else s1], 1)
    w = np.concatenate([wa, wb], 0)
    out = fma_chain(np.zeros((R, w.shape[1]), F32), s, w.T)
    return _swap_tail_rows(out, R) if mut == "rows_swapped_tail" else out


def run_model_pre(b, mut=""):
    H, Kh, R = b["H"], b["Kh"], b["R"]
    wa, wb = b["W0"][:, :Kh], b["W1"][:, H:H + Kh]
    rb, dh = sentinel((R, 2 * H + 3)), sentinel((R, Kh + 3))
    rb[:, :2 * H] = model_pre_fwd(b["h_wide"][:, :Kh], wa, b["ba"], wb, b["bb"], mut)
    dh[:, :Kh] = model_pre_bwd(b["s0_wide"][:, :H], b["s1_wide"][:, :H], wa, wb, mut)
    return rb, dh


# ===================================================================================================== ray_head_fwd / bwd
# (n_out, sigmoid, R, b2 null): n_out in {1, 3, 6, 16}, both activations, R in {1, 2, 31, 32, 33, 65}
HEAD_CASES = [(1, 0, 1, False), (3, 1, 2, False), (6, 0, 31, True), (16, 1, 32, False), (3, 0, 33, False), (16, 0, 65, False),
              (1, 1, 65, False), (6, 1, 33, False)]
HEAD_K0 = 5        # ld_w1 = 64 + K0
HEAD_DENSE = (1, 2)


def _sigmoid64(s):
    return 1.0 / (1.0 + np.exp(-_a(s)))


def ref_head_fwd(rb_wide, w1blk, w2, b2, act, q1, q2):
    """fp64 forward and the per-entry units of the two GEMMs (q1 / q2: the grids of layer 1's / layer 2's products)."""
    rb0, rb1 = _a(rb_wide[:, :64]), _a(rb_wide[:, 64:128])
    a1 = np.maximum(rb0, 0.0)
    a2 = np.maximum(a1 @ _a(w1blk).T + rb1, 0.0)
    pre2 = a2 @ _a(w2).T + (0.0 if b2 is None else _a(b2))
    u1 = _units(w1blk, a1, rb1, q1)
    u2 = _units(w2, a2, None if b2 is None else _a(b2)[None, :], q2)
    return dict(a1=a1, a2=a2, pre2=pre2, out=_sigmoid64(pre2) if act else pre2, u_a2=u1, u_out=u2)


def build_head(C, act, R, dense, b2_null=False, seed=0):
    """dense = 1: W1 7-bit dense, rb 8-bit, W2 rows of <= 3 entries +-1 (a2 is too wide to feed a dense layer 2);
    dense = 2: W1 one +-1 per row, W2 8-bit dense.  The backward's inputs are independent of the forward's outputs: out in
    {1/4, 1/2, 3/4}, dout 4-bit integers, a1 / a2 carrying +0, -0, 2^-126 and ordinary positives."""
    rng = np.random.default_rng(7000 + 100 * C + 10 * R + 2 * dense + act + seed)
    b = dict(C=C, act=act, R=R, dense=dense)
    if dense == 1:
        w1blk, w2 = grid_values(rng, (64, 64), 7, 7), sparse_rows(rng, C, 64, 3, 1.0)
        b2 = grid_values(rng, (C,), 10, 15, nonzero=False)
        q1, q2, qd1, qd0 = 15, 15, 4, 11
    else:
        w1blk, w2 = signed_perm(64, 64, 11 + C + R), grid_values(rng, (C, 64), 8, 8)
        b2 = grid_values(rng, (C,), 20, 16, nonzero=False)
        q1, q2, qd1, qd0 = 8, 16, 12, 12
    b["W1"] = np.ascontiguousarray(np.concatenate([w1blk, grid_values(rng, (64, HEAD_K0), 8, 8)], 1))
    b["W2"], b["b2"] = w2, (None if b2_null else b2)
    b["rb_wide"] = grid_values(rng, (R, 128 + 4), 8, 8, nonzero=False)
    f = ref_head_fwd(b["rb_wide"], w1blk, w2, b["b2"], act, q1, q2)
    assert np.abs(f["pre2"]).max() <= 64.0, "probe broken: the sigmoid's argument leaves the range where its result is a normal number"
    b["fwd"] = f
    # backward
    b["dout"] = grid_values(rng, (R, C), 4, 0, nonzero=False)
    b["y"] = rng.choice(np.array([0.25, 0.5, 0.75], F32), size=(R, C))
    vals = np.array([0.0, -0.0, 2.0 ** -126, 1.0, 0.5, 3.0], F32)
    b["a1m"], b["a2m"] = rng.choice(vals, size=(R, 64)), rng.choice(vals, size=(R, 64))
    d2 = _a(b["dout"]) * _a(b["y"]) * (1.0 - _a(b["y"])) if act else _a(b["dout"])
    d1 = (b["a2m"] > 0) * (d2 @ _a(w2))
    d0 = (b["a1m"] > 0) * (d1 @ _a(w1blk))
    b["bwd"] = dict(dpre2=d2, dpre1=d1, dpre0=d0, u_d1=_units(_a(w2).T, d2, None, qd1), u_d0=_units(_a(w1blk).T, d1, None, qd0))
    return b


def check_head_fwd(b, a1, a2, out, what, report=None):
    f = b["fwd"]
    a1, a2, out = (live_rows(x, b["R"], f"{what} {n}") for x, n in ((a1, "a1"), (a2, "a2"), (out, "out")))
    assert_exact(f"{what} a1", a1, f["a1"], None, 1.0, report)
    assert_exact(f"{what} a2", a2, f["a2"], f["u_a2"], 1.0, report)
    if b["act"]:
        assert (f["u_out"] < BUDGET).all(), "probe broken: the sigmoid's argument is not exact"
        assert_ulp(f"{what} out", out, f["out"], C_SIG)
    else:
        assert_exact(f"{what} out", out, f["out"], f["u_out"], 1.0 if b["dense"] == 2 else 0.0, report)


def check_head_bwd(b, dpre2, dpre1, dpre0, what, report=None):
    w = b["bwd"]
    dpre2, dpre1, dpre0 = (live_rows(x, b["R"], f"{what} {n}") for x, n in ((dpre2, "dpre2"), (dpre1, "dpre1"), (dpre0, "dpre0")))
    assert_exact(f"{what} dpre2", dpre2, w["dpre2"], None, 1.0, report)
    assert_exact(f"{what} dpre1", dpre1, w["dpre1"], w["u_d1"], 1.0, report)
    assert_exact(f"{what} dpre0", dpre0, w["dpre0"], w["u_d0"], 1.0, report)


def model_head_fwd(rb_wide, w1, w2, b2, act, mut=""):
    """a1 = relu(rb0); a2 = relu(chain_k(W1[c][k] a1[k]) from rb1); out = act(chain_k(W2[j][k] a2[k]) from b2)."""
    R, C = rb_wide.shape[0], w2.shape[0]
    p0, p1 = rb_wide[:, :64], rb_wide[:, 64:128]
    if mut == "rb_halves_swapped":
        p0, p1 = p1, p0
    a1 = np.maximum(p0, F32(0)).astype(F32)
    w1blk = w1[:, :64].T if mut == "w1_transposed" else w1[:, :64]
    acc = fma_chain(np.zeros_like(p1) if mut == "rb1_dropped" else p1, a1, w1blk)
    a2 = acc if mut == "a2_no_relu" else np.maximum(acc, F32(0)).astype(F32)
    s0 = np.zeros(C, F32) if (b2 is None or mut == "b2_dropped") else np.asarray(b2, F32)
    s = fma_chain(np.broadcast_to(s0, (R, C)), a2, w2)
    if act:
        e = np.exp(-s.astype(F64)).astype(F32)
        s = (F32(1) / (F32(1) + e).astype(F32)).astype(F32)
    return a1, a2, s


def model_head_bwd(dout, y, a1m, a2m, w1, w2, act, mut=""):
    R = dout.shape[0]
    d = np.asarray(dout, F32)
    if act:
        y = np.asarray(y, F32)
        d = (d * y).astype(F32) if mut == "sigmoid_grad_y" else ((d * y).astype(F32) * (F32(1) - y).astype(F32)).astype(F32)
    if mut == "masks_swapped":
        a1m, a2m = a2m, a1m
    live = (lambda m: m >= 0) if mut == "relu_ge" else (lambda m: m > 0)
    s = fma_chain(np.zeros((R, 64), F32), d, np.asarray(w2, F32).T)
    d1 = np.where(live(a2m), s, F32(0)).astype(F32)
    acc = fma_chain(np.zeros((R, 64), F32), d1, np.asarray(w1[:, :64], F32).T)
    d0 = np.where(live(a1m), acc, F32(0)).astype(F32)
    if mut == "rows_swapped_tail":
        d0 = _swap_tail_rows(d0, R)
    return d, d1, d0


# ================================================================================================================ ray_wgrad
WG_M = [1, 127, 128, 129, 255, 256, 257, 600]
WG_MAX_JOBS = 8
# (n, block widths, bias).  The first WG_MAX_JOBS make a full launch; the rest a launch of several jobs of different n and K.
WG_JOBS = [(1, (1,), True), (3, (15,), False), (15, (16,), True),      # bias column opens k-tile 1
           (16, (63,), True), (17, (64,), True),                         # Kt = 64 exactly / bias column opens k-tile 4
           (64, (64,), False),                                           # ... next to the same block without a bias
           (64, (64, 63), True),                                         # the full 8 k-tiles (Kx = 127 + the ones column)
           (16, (64, 48), True),                                         # Kx = 112: the ones column opens k-tile 7
           (3, (64, 48), False),                                         # ... and is absent
           (17, (1, 1), True), (64, (16,), False), (15, (15,), True)]   # blocks (1, 1); Kt = 16 exactly
WG_QDY, WG_QX = 5, 6


def build_wgrad(M, preload, seed=0):
    """5-bit dy on 2^-5, 6-bit x on 2^-6 (<= 600 rows x 2^11 units), targets preloaded on the product grid (20 bits) or zero.
    Operands carry one guard row past M (never handed to the kernel's row count: what an off-by-one tail clamp would read)."""
    rng = np.random.default_rng(31 * M + preload + seed)
    jobs = []
    q = WG_QDY + WG_QX
    for n, widths, bias in WG_JOBS:
        j = dict(n=n, widths=widths, bias=bias, M=M)
        j["dy_wide"] = grid_values(rng, (M + 1, n + 2), WG_QDY, WG_QDY, nonzero=False)
        j["x_wide"] = [grid_values(rng, (M + 1, w + 3), WG_QX, WG_QX, nonzero=False) for w in widths]
        dst, col = [], 2
        for w in widths:
            dst.append(col)
            col += w + 3
        j["dst"] = dst
        ld = col - 2
        pre = grid_values(rng, (n, ld), 20, q) if preload else np.zeros((n, ld), F32)
        touched = np.zeros(ld, bool)
        for w, d in zip(widths, dst):
            touched[d:d + w] = True
        j["touched"] = touched
        dw0 = sentinel((n, ld))
        dw0[:, touched] = pre[:, touched]
        j["dw0"] = dw0
        j["db0"] = (grid_values(rng, (n,), 20, q) if preload else np.zeros(n, F32)) if bias else None
        dy = _a(j["dy_wide"][:M, :n])
        ref, un = np.zeros((n, ld)), np.zeros((n, ld))
        for xw, w, d in zip(j["x_wide"], widths, dst):
            x = _a(xw[:M, :w])
            ref[:, d:d + w] = _a(pre[:, d:d + w]) + dy.T @ x
            un[:, d:d + w] = (np.abs(dy).T @ np.abs(x) + np.abs(_a(pre[:, d:d + w]))) * 2.0 ** q
        j["dw"], j["u_dw"] = ref, un
        if bias:
            j["db"] = _a(j["db0"]) + dy.sum(0)
            j["u_db"] = (np.abs(dy).sum(0) + np.abs(_a(j["db0"]))) * 2.0 ** q
        jobs.append(j)
    return jobs


def check_wgrad(j, dw, db, what, report=None):
    t = j["touched"]
    dw = live_rows(dw, j["n"], f"{what} dw")
    assert is_sentinel(np.asarray(dw)[:, ~t]), f"{what}: columns of dw outside the job's blocks were written"
    assert_exact(f"{what} dw", np.asarray(dw)[:, t], j["dw"][:, t], j["u_dw"][:, t], 1.0, report)
    if j["bias"]:
        assert_exact(f"{what} db", db, j["db"], j["u_db"], 1.0, report)


def model_wgrad(j, mut=""):
    """One job in the kernel's order: per 256-row chunk, quarter q of the sixteen waves accumulates rows 32q .. 32q+31 of each
    128-row round (MFMA steps of four rows; modelled as one fmaf per row), quarters 2, 3 are added to 0, 1, quarter 1 to 0, and
    the chunk's sums leave with one float atomic per target entry."""
    M, n, widths, bias = j["M"], j["n"], j["widths"], j["bias"]
    Kx = sum(widths)
    has_b = bias and not (mut == "bias_dropped_at_16" and Kx % 16 == 0)
    Kt = Kx + (1 if has_b else 0)
    KT = Kt // 16 if mut == "ktiles_floor" else -(-Kt // 16)
    ones = np.full((M + 1, 1), 0.0 if mut == "no_ones_column" else 1.0, F32)
    X = np.concatenate([xw[:, :w] for xw, w in zip(j["x_wide"], widths)] + [ones], 1).astype(F64)
    dy = j["dy_wide"][:, :n].astype(F64)
    dw = np.array(j["dw0"], F32)
    db = None if not bias else np.array(j["db0"], F32)
    for chunk in range(-(-M // 256)):
        acc = np.zeros((4, n, Kx + 1), F32)
        for rnd in range(2):
            r0 = chunk * 256 + rnd * 128
            if r0 >= M or (mut == "second_round_dropped" and rnd == 1):
                break
            last = M - 1 - r0 + (1 if mut == "tail_clamp_row_M" else 0)
            for rr in range(min(128, last + 1)):
                qd = rr // 32
                acc[qd] = (acc[qd].astype(F64) + dy[r0 + rr][:, None] * X[r0 + rr][None, :]).astype(F32)
        lo = (acc[0] + acc[2]).astype(F32)
        hi = acc[1] if mut == "quarter_3_dropped" else (acc[1] + acc[3]).astype(F32)
        tot = (lo + hi).astype(F32)
        for k in range(min(Kt, 16 * KT)):
            if k < widths[0]:
                col = j["dst"][0] + k
            elif k < Kx:
                col = (j["dst"][0] + k) if mut == "dst_col_1_ignored" else (j["dst"][1] + k - widths[0])
            else:
                db[:] = tot[:, k] if mut == "target_overwritten" else (db + tot[:, k]).astype(F32)
                continue
            dw[:, col] = tot[:, k] if mut == "target_overwritten" else (dw[:, col] + tot[:, k]).astype(F32)
    return dw, db


# =============================================================================================================== embed_grad
# (R, n_emb, E, which gradients): one, two and three scan rounds of 8192 rays; n_emb = 1 at R = 8192 fills every wave's list
EMB_CASES = [(1, 1, 1, "a"), (63, 3, 5, "ab"), (64, 1000, 16, "ab"), (65, 3, 17, "b"), (8191, 3, 20, "ab"), (8192, 1, 16, "ab"),
             (8193, 1000, 33, "ab"), (16500, 1, 20, "ab")]
EMB_P = 3          # the gradients are column blocks [P : P + E] of wider rows
EMB_Q = 6


def build_embed(R, n_emb, E, which, seed=0):
    """6-bit gradients on 2^-6 (<= 16500 x 2 x 2^6 units), dw preloaded with non-zero 20-bit values on the same grid.  Indices
    are column 1 of an [R, 2] tensor; outside the full-list case a few are negative or >= n_emb, and with n_emb = 3 no ray
    uses row 1."""
    rng = np.random.default_rng(17 * R + n_emb + E + seed)
    b = dict(R=R, n_emb=n_emb, E=E, which=which)
    idx = rng.integers(0, n_emb, size=R)
    if n_emb == 3:
        idx = rng.choice(np.array([0, 2]), size=R)
    full = n_emb == 1 and R == 8192
    if R >= 8 and not full:
        bad = rng.random(R) < 0.05
        idx = np.where(bad, rng.choice(np.array([-1, -7, n_emb, n_emb + 5]), size=R), idx)
        idx[R // 2], idx[R - 1] = -1, n_emb
    b["idx_wide"] = np.stack([rng.integers(0, n_emb, size=R), idx], 1).astype(np.int64)
    b["ga_wide"] = grid_values(rng, (R, EMB_P + E), EMB_Q, EMB_Q, nonzero=False) if "a" in which else None
    b["gb_wide"] = grid_values(rng, (R, EMB_P + E + 1), EMB_Q, EMB_Q, nonzero=False) if "b" in which else None
    b["dw0"] = grid_values(rng, (n_emb, E), 20, EMB_Q)
    g, mag = np.zeros((R, E)), np.zeros((R, E))
    for k in ("ga_wide", "gb_wide"):
        if b[k] is not None:
            g += _a(b[k][:, EMB_P:EMB_P + E])
            mag += np.abs(_a(b[k][:, EMB_P:EMB_P + E]))
    ok = (idx >= 0) & (idx < n_emb)
    ref, un = _a(b["dw0"]).copy(), np.abs(_a(b["dw0"]))
    np.add.at(ref, idx[ok], g[ok])
    np.add.at(un, idx[ok], mag[ok])
    b["dw"], b["u_dw"] = ref, un * 2.0 ** EMB_Q
    b["unused"] = np.setdiff1d(np.arange(n_emb), idx[ok])
    return b


def check_embed(b, dw, what, report=None):
    dw = np.asarray(dw, F32)
    u = b["unused"]
    assert np.array_equal(dw[u].view(np.uint32), b["dw0"][u].view(np.uint32)), f"{what}: a row no ray uses changed"
    assert_exact(f"{what} dw", dw, b["dw"], b["u_dw"], 1.0, report)


def model_embed(b, mut=""):
    """Per table row: sixteen waves compact the matching rays of a scan round (8192 rays; wave w sees rays u 1024 + 64 w + lane)
    into lists in scan order, lane l adds entries l, l + 128, ... paired with l + 64, ... as (ga + gb) + (ga' + gb'); a xor
    butterfly over the lanes, a fixed-order sum over the waves, one add onto dw.  Column chunks of 16 are independent."""
    R, n_emb, E = b["R"], b["n_emb"], b["E"]
    idx = b["idx_wide"][:, 1].copy()
    if mut == "out_of_range_folded":
        idx = np.clip(idx, 0, n_emb - 1)
    ga = np.zeros((R, E), F32) if b["ga_wide"] is None else b["ga_wide"][:, EMB_P:EMB_P + E]
    gb = np.zeros((R, E), F32) if b["gb_wide"] is None else b["gb_wide"][:, EMB_P:EMB_P + E]
    dw = np.array(b["dw0"], F32)
    order = np.argsort(idx, kind="stable")
    rows, starts = np.unique(idx[order], return_index=True)
    ends = list(starts[1:]) + [R]
    lanes = np.arange(64)
    for row, s, e in zip(rows, starts, ends):
        if row < 0 or row >= n_emb:
            continue
        rays = order[s:e]
        acc = np.zeros((16, 64, E), F32)
        for sbase in range(0, R, 8192):
            if mut == "second_scan_round_dropped" and sbase > 0:
                break
            loc = rays[(rays >= sbase) & (rays < sbase + 8192)] - sbase
            wave = (loc % 1024) // 64
            for w in np.unique(wave):
                lst = loc[wave == w]                      # ascending ray = (u, lane) scan order
                if mut == "list_beyond_511_dropped":
                    lst = lst[:511]
                cnt = lst.size
                for t in range(0, cnt, 128):
                    i = lanes + t
                    on = i < cnt
                    two = on & (i + 64 < cnt)
                    ra = sbase + lst[np.where(on, i, 0)]
                    rb = sbase + lst[np.where(two, i + 64, 0)]
                    first = (ga[ra] + gb[ra]).astype(F32)
                    second = np.where(two[:, None], (ga[rb] + (F32(0) if mut == "paired_gb_dropped" else gb[rb])).astype(F32), F32(0)).astype(F32)
                    add = np.where(on[:, None], (first + second).astype(F32), F32(0)).astype(F32)
                    acc[w] = (acc[w] + add).astype(F32)
        for off in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, lanes ^ off]).astype(F32)
        tot = np.zeros(E, F32)
        for w in range(16):
            tot = (tot + acc[w, 0]).astype(F32)
        if mut == "columns_from_16_dropped":
            tot[16:] = 0
        dw[row] = tot if mut == "target_overwritten" else (dw[row] + tot).astype(F32)
    return dw


# ============================================================================================== direction rows (sinf columns)
DIR_DEGS = [0, 3, 4, 10]
DIR_N = [1, 255, 257, 1000]
HALF_PI = F32(0.5) * F32(3.14159265358979323846)


def build_dirs(n, seed=0):
    """Unit directions, then rows with components exactly 0 and +-1, then rows on the 2^-10 grid (not normalised: the kernels
    do not require it).  Returns (dirs fp32 [n, 3], mask of the rows on the grid)."""
    rng = np.random.default_rng(500 + n + seed)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    special = np.array([[0, -1, 1], [1, 0, 0], [0, 0, -1], [-1, 1, 0], [0, 0, 0], [1, 1, 1], [-1, -1, -1]], F32)
    grid = np.zeros(n, bool)
    k = min(n, len(special))
    d[:k], grid[:k] = special[:k], True
    m = min(max(n - k, 0), max(n // 4, 1)) if n > k else 0
    if m:
        d[k:k + m] = rng.integers(-1024, 1025, size=(m, 3)) * F32(2.0 ** -10)
        grid[k:k + m] = True
    return d, grid


def dir_width(max_deg):
    return 3 if max_deg == 0 else 3 * (1 + 2 * (max_deg + 1))


def restate_dir_rows(dirs, max_deg, remap, mut=""):
    """(identity columns fp32 [n, 3], fp32 arguments of the sin columns [n, width - 3]) as the kernels form them:
    x = (d + 1) / 2 or d; argument x 2^k (exact), then + half_pi (both fp32) for the second half."""
    d = np.asarray(dirs, F32)
    if mut == "raw_and_remapped_exchanged":
        remap = not remap
    x = ((d + F32(1)).astype(F32) / F32(2)).astype(F32) if remap else d
    if max_deg == 0:
        return x, np.zeros((d.shape[0], 0), F32)
    n_deg = max_deg + 1
    sc = np.exp2(np.arange(n_deg) + (1 if mut == "degree_off_by_one" else 0)).astype(F32)
    xb = (x[:, None, :] * sc[None, :, None]).astype(F32).reshape(d.shape[0], 3 * n_deg)
    if mut == "half_pi_in_double":
        sh = (xb.astype(F64) + np.pi / 2).astype(F32)
    else:
        sh = (xb + HALF_PI).astype(F32)
    return x, np.concatenate([xb, sh], 1)


def ulp32(ref):
    """The fp32 unit in the last place at |ref| (2^-149 below the normal range)."""
    _, e = np.frexp(np.abs(_a(ref)))
    return np.exp2(np.maximum(e - 1, -126).astype(F64) - 23)


def check_dir_rows(got, dirs, grid, max_deg, remap, e_sinf, what):
    """Identity columns bitwise (against the exact fp64 value on the grid rows); sin columns within e_sinf ulps of the fp64 sin
    of the fp32 argument.  Prints and returns the worst error in ulps."""
    got = np.asarray(got, F32)
    x, args = restate_dir_rows(dirs, max_deg, remap)
    assert got.shape == (x.shape[0], dir_width(max_deg)), f"{what}: shape {got.shape}"
    assert np.array_equal(got[:, :3].view(np.uint32), x.view(np.uint32)), f"{what}: identity columns differ"
    exact = (_a(dirs) + 1.0) / 2.0 if remap else _a(dirs)
    assert np.array_equal(_a(got[grid, :3]), exact[grid]), f"{what}: identity columns of the grid rows are not exact"
    if args.shape[1] == 0:
        return 0.0
    ref = np.sin(args.astype(F64))
    err = np.abs(_a(got[:, 3:]) - ref) / ulp32(ref)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"\n[sinf] {what}: worst {err[i]:.3f} ulp at argument {args[i]!r} (bound {e_sinf} ulp)")
    assert (err <= e_sinf).all(), f"{what}: sin column {i[1]} of row {i[0]}: {err[i]:.3f} ulp from sin({args[i]!r}) (bound {e_sinf})"
    return float(err[i])


def model_dir_rows(dirs, max_deg, remap, mut=""):
    x, args = restate_dir_rows(dirs, max_deg, remap, mut)
    return np.concatenate([x, np.sin(args.astype(F64)).astype(F32)], 1)


def sinf_sweep(log2n=21, seed=0):
    """fp32 arguments (a multiple of 3 of them) spanning what max_deg <= 10 can form from |x| <= 1, both signs: uniform in
    [-1026, 1026] and in [-2, 2], log-spaced magnitudes from 2^-40, the +-1600 fp32 neighbours of every zero crossing k pi
    and every eighth neighbour of every extremum up to 326 pi (thinned below log2n = 21), the 2^-10 grid times 2^k, and
    x 2^k of uniform x.  emer_dir_encode(remap off, max_deg = 1) evaluates sinf at a, 2 a, fl(a + hp) and fl(2 a + hp)."""
    rng = np.random.default_rng(seed)
    n = 1 << log2n
    parts = [rng.uniform(-1026.0, 1026.0, n), rng.uniform(-2.0, 2.0, n)]
    mag = np.exp2(rng.uniform(-40.0, np.log2(1026.0), n // 2))
    parts.append(mag * rng.choice([-1.0, 1.0], n // 2))
    k = np.arange(0, 327)
    j = np.arange(-1600, 1601, max(1, 1 << max(0, 21 - log2n)))
    near = (k * np.pi).astype(F32).view(np.int32)[:, None] + j[None, :]
    near = np.where(near < 0, 0, near).astype(np.int32).view(F32).reshape(-1)   # (k = 0: zero and the smallest subnormals)
    parts += [near.astype(F64), -near.astype(F64)]
    ext = ((k + 0.5) * np.pi).astype(F32).view(np.int32)[:, None] + j[None, ::8]
    parts.append(ext.astype(np.int32).view(F32).reshape(-1).astype(F64))
    parts.append(((np.arange(-1024, 1025) * 2.0 ** -10)[:, None] * (2.0 ** np.arange(11))[None, :]).reshape(-1))
    x = rng.uniform(-1.0, 1.0, n).astype(F32)
    parts.append((x * np.exp2(rng.integers(0, 11, n)).astype(F32)).astype(F64))
    a = np.concatenate(parts).astype(F32)
    return np.concatenate([a, np.zeros((-a.size) % 3, F32)])


def sinf_sweep_error(a, out):
    """out = emer_dir_encode(a as [n, 3], max_deg 1, remap off) -> the worst error of its twelve sin columns in ulps."""
    x = np.asarray(a, F32).reshape(-1, 3)
    _, args = restate_dir_rows(x, 1, False)
    ref = np.sin(args.astype(F64))
    got = _a(np.asarray(out, F32)[:, 3:])
    err = np.abs(got - ref) / ulp32(ref)
    i = np.unravel_index(int(np.argmax(err)), err.shape)
    return dict(n_args=int(args.size), max_ulp=float(err[i]), at=float(args[i]), got=float(got[i]), ref=float(ref[i]),
                max_abs=float(np.abs(got - ref).max()), not_correctly_rounded=float((got != _a(ref.astype(F32))).mean()))


# ============================================================================================================ forward chain
CHAIN_R = [1, 33, 65]
CHAIN_E, CHAIN_NEMB = 16, 3


def build_chain(R, seed=0):
    """inputs (max_deg = 0: rows [d | emb[idx]]) -> pre_fwd -> head_fwd, exact end to end: 8-bit directions and embedding on
    2^-8, W0 and W1's input block 8-bit, W1's hidden block one +-1 per row, W2 rows of <= 3 entries +-1."""
    rng = np.random.default_rng(900 + R + seed)
    E, Kh = CHAIN_E, 3 + CHAIN_E
    b = dict(R=R, Kh=Kh, E=E, n_emb=CHAIN_NEMB)
    b["dirs"] = grid_values(rng, (R, 3), 8, 8, nonzero=False)
    b["emb"] = grid_values(rng, (CHAIN_NEMB, E), 8, 8)
    b["idx"] = rng.integers(0, CHAIN_NEMB, size=R).astype(np.int64)
    b["W0"], b["b0"] = grid_values(rng, (64, Kh), 8, 8), grid_values(rng, (64,), 20, 16, nonzero=False)
    b["W1"] = np.ascontiguousarray(np.concatenate([signed_perm(64, 64, 3 + R), grid_values(rng, (64, Kh), 8, 8)], 1))
    b["b1"] = grid_values(rng, (64,), 20, 16, nonzero=False)
    b["W2"], b["b2"] = sparse_rows(rng, 3, 64, 3, 1.0), grid_values(rng, (3,), 10, 16, nonzero=False)
    x = np.concatenate([_a(b["dirs"]), _a(b["emb"])[b["idx"]]], 1)
    b["x_sky"] = x
    b["x_rgb"] = np.concatenate([(_a(b["dirs"]) + 1.0) / 2.0, _a(b["emb"])[b["idx"]]], 1)
    wa, wb = b["W0"], b["W1"][:, 64:]
    b["rb"] = np.concatenate([x @ _a(wa).T + _a(b["b0"]), x @ _a(wb).T + _a(b["b1"])], 1)
    b["u_rb"] = np.concatenate([_units(wa, x, b["b0"], 16), _units(wb, x, b["b1"], 16)], 1)
    assert (b["u_rb"] < BUDGET).all()
    b["fwd"] = ref_head_fwd(b["rb"], b["W1"][:, :64], b["W2"], b["b2"], 1, 16, 16)
    assert np.abs(b["fwd"]["pre2"]).max() <= 64.0
    b["act"], b["dense"] = 1, 1
    return b


def check_chain(b, x_sky, rb, a1, a2, out, what, report=None):
    assert_exact(f"{what} rows", live_rows(x_sky, b["R"], f"{what} rows"), b["x_sky"], None, 1.0, report)
    assert_exact(f"{what} rb", live_rows(rb, b["R"], f"{what} rb"), b["rb"], b["u_rb"], 1.0, report)
    check_head_fwd(b, a1, a2, out, what, report)


def model_chain(b, mut=""):
    d = b["dirs"] if mut != "raw_and_remapped_exchanged" else ((b["dirs"] + F32(1)) / F32(2)).astype(F32)
    x = np.concatenate([d, b["emb"][b["idx"]]], 1).astype(F32)
    rb = model_pre_fwd(x, b["W0"], b["b0"], b["W1"][:, 64:], b["b1"], mut)
    a1, a2, out = model_head_fwd(rb, b["W1"], b["W2"], b["b2"], 1, mut)
    return x, rb, a1, a2, out


# ================================================================================================================== mutants
# name -> (family whose probes must catch it, what the slip is)
MUTANTS = {
    "tail_clamp_row_M": ("wgrad", "the tail row clamp reads row M instead of M - 1 (and counts it live)"),
    "no_ones_column": ("wgrad", "the ones column of the bias is missing"),
    "dst_col_1_ignored": ("wgrad", "the second block lands behind the first: its dst_col is ignored"),
    "bias_dropped_at_16": ("wgrad", "the bias column is dropped when Kx % 16 == 0"),
    "ktiles_floor": ("wgrad", "Kx / 16 k-tiles instead of the ceiling"),
    "second_round_dropped": ("wgrad", "rows 128 .. 255 of a chunk are not accumulated"),
    "quarter_3_dropped": ("wgrad", "the fold leaves out the fourth row quarter"),
    "target_overwritten": ("wgrad", "a chunk's sums are stored instead of added"),
    "relu_ge": ("head_bwd", ">= 0 ReLU masks"),
    "masks_swapped": ("head_bwd", "the a1 and a2 masks exchanged"),
    "sigmoid_grad_y": ("head_bwd", "sigmoid' as y instead of y (1 - y)"),
    "rows_swapped_tail": ("head_bwd", "rows 2q and 2q + 1 exchanged in the tail tile"),
    "rb_halves_swapped": ("head_fwd", "the two halves of rb exchanged"),
    "w1_transposed": ("head_fwd", "W1's hidden block read transposed"),
    "rb1_dropped": ("head_fwd", "layer 1 starts from zero instead of rb1"),
    "a2_no_relu": ("head_fwd", "a2 without its ReLU"),
    "b2_dropped": ("head_fwd", "b2 not added"),
    "pre_halves_swapped": ("pre", "rb's halves written in each other's place"),
    "pre_bias_b_from_a": ("pre", "the second half's bias read from ba"),
    "pre_bwd_s1_dropped": ("pre", "d h without the s1 W1 share"),
    "list_beyond_511_dropped": ("embed", "embed_grad drops list entries beyond 511"),
    "second_scan_round_dropped": ("embed", "embed_grad stops after the first scan round of 8192 rays"),
    "columns_from_16_dropped": ("embed", "embed_grad drops the columns >= 16"),
    "paired_gb_dropped": ("embed", "embed_grad drops the g_b addend of the paired row"),
    "out_of_range_folded": ("embed", "out-of-range indices folded into rows 0 / n_emb - 1"),
    "raw_and_remapped_exchanged": ("dirs", "raw and remapped direction rows exchanged"),
    "degree_off_by_one": ("dirs", "scales 2^(k+1) instead of 2^k"),
    "half_pi_in_double": ("dirs", "x 2^k + pi/2 formed in double and rounded once"),
}
