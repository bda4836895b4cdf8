"""The generic MLP chain kernel (mlp_chain_kernel / emer_mlp_chain, csrc/mlp.hip) as plain Python: its launch plan, an fp64
executor of a chain descriptor, three mutants of that executor and the probe cases (test helper, not a test module).

``plan`` is a RESTATEMENT of chain_lds_plan and of the wave-count loop of emer_mlp_chain and must follow the kernel: the
tests use it to decide which branch a case reaches (column groups, K % 8 tails, fewer than 16 waves, a second pass of the
persistent grid), never to compute an expected value.

``run_ref`` evaluates a descriptor at the LOGICAL level: a row's buffer starts at zero, segments fill it, and every layer
reads its whole input (K columns from in_col) before it writes act(x W^T + b) [+ old value] [masked] to N columns from
out_col.  The chain runs fp32-input MFMA, a k-permuted fmaf chain per output entry, so the only exactness condition is the
one tests/_head_probe.py states: operands on a fixed-point grid and sum |a| |b| + |bias| (+ |accumulated value|) below 2^24
units per entry; then every partial sum in any order is exact and a correct kernel returns the fp64 result bit for bit.
``run_ref`` reports those units per stored entry.

Mutants (``mutant=``), each a way the kernel could be wrong that a 64-wide, single-pass, K % 8 == 0 suite cannot see:
  "overlap"    a column group >= 1 re-reads the row buffer, so it sees the outputs of the groups before it where the
               layer's input and output regions overlap;
  "drop_tail"  the K % 8 tail of a layer's reduction is dropped;
  "acc_prev"   ``accumulate`` adds what the buffer column held at the end of the wave's PREVIOUS tile (row - rows_per_pass).
``stale=True`` is not a mutant but the kernel's own buffer model: the buffer is kept from a wave's previous tile and a layer
multiplies the round_up(K, 8) - K columns past its input by zero weights -- 0 for finite leftovers, NaN for an inf.
"""
import numpy as np

from tests import _head_probe as P

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TRUNC_EXP = 0, 1, 2, 3
E15 = float(np.float32(np.exp(15.0)))
LDS_BYTES, MAX_COLS, GRID = 160 * 1024, 512, 256
MUTANTS = ("overlap", "drop_tail", "acc_prev")


def _ru(x, m):
    return -(-x // m) * m


# ------------------------------------------------------------------------------------------------------------ launch plan
def plan(buf_cols: int, kn) -> dict:
    """chain_lds_plan + the launch arithmetic of emer_mlp_chain for layers kn = [(K, N), ...] (restated; follows the kernel)."""
    kpad = [_ru(K, 8) for K, _ in kn]
    npad = [_ru(N, 16) for _, N in kn]
    w_pitch = [k + 2 for k in kpad]
    off = 0
    for n, p in zip(npad, w_pitch):
        off += n * p + n          # weights, then the bias
    w_total = _ru(off, 4)
    Pp = _ru(buf_cols + 8, 4) + 2
    n_waves = 16
    while n_waves > 4 and (w_total + n_waves * 16 * Pp) * 4 > LDS_BYTES:
        n_waves -= 2
    lds = (w_total + n_waves * 16 * Pp) * 4
    return {"kpad": kpad, "npad": npad, "ntiles": [n // 16 for n in npad], "w_pitch": w_pitch, "w_total": w_total, "P": Pp,
            "n_waves": n_waves, "lds": lds, "rows_per_pass": GRID * n_waves * 16,
            "lds4": (w_total + 4 * 16 * Pp) * 4, "fits": 4 <= buf_cols <= MAX_COLS and lds <= LDS_BYTES}


def plan_of(segs, layers, buf_cols) -> dict:
    return plan(buf_cols, [_eff_w(L).shape[::-1] for L in layers])


# ------------------------------------------------------------------------------------------------------------ descriptors
def rm(data, col, width=None, row_div=1, fix_a=None, fix_b=None):
    """Row-major segment: value(row, c) = data[row // row_div, c] for c < width (data may be wider: ld > width)."""
    data = np.asarray(data, np.float32)
    return {"mode": 0, "data": data, "col": col, "width": data.shape[1] if width is None else width, "row_div": row_div,
            "fix_a": fix_a, "fix_b": fix_b}


def lm(data, col):
    """Level-major segment [L, N, f] as L * f columns."""
    data = np.asarray(data, np.float32)
    return {"mode": 1, "data": data, "col": col, "width": data.shape[0] * data.shape[2]}


def lay(w, bias, in_col, out_col, act=ACT_NONE, transposed=False, n_slice=None, mask=None, store=None, store_cols=None,
        store_lm=0, store_ld=None, store_exp0=False, accumulate=False):
    """w is a Linear weight [out, in] (fused.layer's convention).  store: the name the stored columns get in the result;
    store_lm = f > 0: stored level-major [n / f, rows, f]; store_ld: row pitch of the store target (> its width)."""
    return {"w": np.asarray(w, np.float32), "bias": None if bias is None else np.asarray(bias, np.float32), "in_col": in_col,
            "out_col": out_col, "act": act, "transposed": transposed, "n_slice": n_slice,
            "mask": None if mask is None else np.asarray(mask, np.float32), "store": store, "store_cols": store_cols,
            "store_lm": store_lm, "store_ld": store_ld, "store_exp0": store_exp0, "accumulate": accumulate}


def _eff_w(L):
    """[N, K] weights the layer multiplies with (transposed / n_slice applied)."""
    w = L["w"].T if L["transposed"] else L["w"]
    a, b = L["n_slice"] if L["n_slice"] is not None else (0, w.shape[0])
    return w[a:b]


def _eff_b(L):
    if L["bias"] is None:
        return None
    a, b = L["n_slice"] if L["n_slice"] is not None else (0, L["bias"].shape[0])
    return L["bias"][a:b]


def _act(act, pre):
    with np.errstate(over="ignore"):
        if act == ACT_RELU:
            return np.maximum(pre, 0.0)
        if act == ACT_SIGMOID:
            return 1.0 / (1.0 + np.exp(-pre))
        if act == ACT_TRUNC_EXP:   # exp of the fp32 value of pre - 1, inf past fp32 (tests/test_head_exact_gpu.py::_trunc_ref)
            d = np.exp((pre.astype(np.float32) - np.float32(1.0)).astype(np.float64))
            return np.where(d > np.finfo(np.float32).max, np.inf, d)
    return pre


def _fill(segs, r0, r1, buf):
    for S in segs:
        if S["mode"] == 1:
            d = S["data"][:, r0:r1, :].astype(np.float64)
            buf[:, S["col"]:S["col"] + S["width"]] = d.transpose(1, 0, 2).reshape(r1 - r0, -1)
        else:
            src = np.arange(r0, r1) // S["row_div"]
            buf[:, S["col"]:S["col"] + S["width"]] = S["data"][src, :S["width"]].astype(np.float64)
            if S["fix_a"] is not None:
                buf[:, S["col"]] += np.asarray(S["fix_a"], np.float64)[r0:r1] * np.minimum(np.asarray(S["fix_b"], np.float64)[r0:r1], E15)


def _units(x, w, b, old):
    """sum |x| |w| + |bias| + |old| in units of the finest grid the operands lie on (inf where an operand is not finite)."""
    if not (np.isfinite(x).all() and np.isfinite(w).all()):
        return np.full((x.shape[0], w.shape[0]), np.inf)
    q = P.grid_of(x) + P.grid_of(w)
    u = np.abs(x) @ np.abs(w).T
    for extra in (b, old):
        if extra is not None:
            if not np.isfinite(extra).all():
                return np.full(u.shape, np.inf)
            q = max(q, P.grid_of(extra))
            u = u + np.abs(extra)
    return u * 2.0 ** q


def run_ref(segs, layers, buf_cols, n_rows, mutant=None, stale=False, rows_per_pass=None):
    """fp64 result of the descriptor: {store name: values, name + ":pre": the pre-activations of the stored columns,
    name + ":units": their exact-budget units, name + ":exp0": the value whose exp(. - 1) store_exp0 writes}."""
    assert mutant in (None,) + MUTANTS
    rpp = rows_per_pass or plan_of(segs, layers, buf_cols)["rows_per_pass"]
    width = buf_cols + 16
    out = {}
    prev = None
    for r0 in range(0, n_rows, rpp):
        r1 = min(r0 + rpp, n_rows)
        m = r1 - r0
        buf = np.zeros((m, width))
        if stale and prev is not None:
            buf[:] = prev[:m]
        _fill(segs, r0, r1, buf)
        for L in layers:
            w, b = _eff_w(L).astype(np.float64), _eff_b(L)
            N, K = w.shape
            i0, o0 = L["in_col"], L["out_col"]
            keff = K - K % 8 if mutant == "drop_tail" else K
            old = buf[:, o0:o0 + N].copy()
            if mutant == "acc_prev":
                old = np.zeros((m, N)) if prev is None else prev[:m, o0:o0 + N]
            x = buf[:, i0:i0 + K].copy()
            pre, val = np.empty((m, N)), np.empty((m, N))
            for c0 in range(0, N, 64):   # the kernel's column groups; only the "overlap" mutant can tell them apart
                if mutant == "overlap":
                    x = buf[:, i0:i0 + K].copy()
                c1 = min(c0 + 64, N)
                with np.errstate(invalid="ignore"):
                    p = x[:, :keff] @ w[c0:c1, :keff].T + (0.0 if b is None else b[c0:c1].astype(np.float64))
                    if stale:   # the zero-weight columns past K: 0 * leftover
                        p = p + (0.0 * buf[:, i0 + K:i0 + _ru(K, 8)]).sum(1)[:, None]
                    v = _act(L["act"], p)
                    if L["accumulate"]:
                        v = v + old[:, c0:c1]
                if L["mask"] is not None:
                    v = np.where(L["mask"][r0:r1, c0:c1] > 0, v, 0.0)
                pre[:, c0:c1], val[:, c0:c1] = p, v
                if mutant == "overlap":
                    buf[:, o0 + c0:o0 + c1] = v
            buf[:, o0:o0 + N] = val
            name = L["store"]
            if name is not None:
                a, e = L["store_cols"] if L["store_cols"] is not None else (0, N)
                val = buf[:, o0 + a:o0 + e]
                un = _units(x, w[a:e], None if b is None else b[a:e], None)
                for key, blk in ((name, val), (name + ":pre", pre[:, a:e]), (name + ":units", un)):
                    out.setdefault(key, []).append(blk.copy())
            if L["store_exp0"]:
                out.setdefault((name or "layer") + ":exp0", []).append(buf[:, o0].copy())
        prev = buf
    res = {k: np.concatenate(v, 0) for k, v in out.items()}
    for L in layers:
        if L["store"] is not None and L["store_lm"]:
            f = L["store_lm"]
            for key in (L["store"], L["store"] + ":pre", L["store"] + ":units"):
                res[key] = res[key].reshape(n_rows, -1, f).transpose(1, 0, 2)
    return res


def accumulate_units(segs, layers, buf_cols, n_rows, res):
    """Adds |value accumulated onto| to the units of the accumulate layers' stores (their sum must stay inside the budget too):
    the accumulated-onto block is the stored value minus this layer's own product."""
    for L in layers:
        if L["accumulate"] and L["store"] is not None and not L["store_lm"]:
            n = L["store"]
            q = max(P.grid_of(res[n]), P.grid_of(res[n + ":pre"]))
            res[n + ":units"] = res[n + ":units"] + np.abs(res[n] - res[n + ":pre"]) * 2.0 ** q
    return res


# ------------------------------------------------------------------------------------------------------------ GPU runner
def run_gpu(segs, layers, buf_cols, n_rows, dev="cuda:0"):
    """The same descriptor through fused.seg / seg_lm / layer / run_chain; returns {store name: numpy, name + ":exp0": numpy}."""
    import torch
    from emernerf_amd import fused
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(dev)
    keep, gs, gl, outs = [], [], [], {}
    for S in segs:
        d = t(S["data"]); keep.append(d)
        if S["mode"] == 1:
            s = fused.seg_lm(d, S["col"])
        else:
            s = fused.seg(d[:, :S["width"]], S["col"], S["width"], ld=d.stride(0), row_div=S["row_div"])
            if S["fix_a"] is not None:
                fa, fb = t(S["fix_a"]), t(S["fix_b"]); keep += [fa, fb]
                s.fix_a, s.fix_b = fa.data_ptr(), fb.data_ptr()
        gs.append(s)
    for L in layers:
        w, b, mk = t(L["w"]), t(L["bias"]), t(L["mask"]); keep += [w, b, mk]
        N = _eff_w(L).shape[0]
        a, e = L["store_cols"] if L["store_cols"] is not None else (0, N)
        st = ex = None
        if L["store"] is not None:
            if L["store_lm"]:
                st = torch.full(((e - a) // L["store_lm"], n_rows, L["store_lm"]), float("nan"), device=dev)
                outs[L["store"]] = st
            else:
                full = torch.full((n_rows, L["store_ld"] or (e - a)), float("nan"), device=dev)
                st = full   # the kernel writes the first e - a columns of each row; the rest must stay untouched
                outs[L["store"]], outs[L["store"] + ":full"] = full[:, :e - a], full
        if L["store_exp0"]:
            ex = torch.full((n_rows,), float("nan"), device=dev)
            outs[(L["store"] or "layer") + ":exp0"] = ex
        gl.append(fused.layer(w, b, L["in_col"], L["out_col"], L["act"], transposed=L["transposed"], n_slice=L["n_slice"], mask=mk,
                              store=st, store_cols=L["store_cols"], store_lm=bool(L["store_lm"]), store_exp0=ex,
                              accumulate=L["accumulate"]))
    fused.run_chain(gs, gl, buf_cols, n_rows, keep[0])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


# ------------------------------------------------------------------------------------------------------------ case tables
def _r4(x):
    return _ru(x, 4)


def one_layer(kind, K, N, rows, row_div=1, seed=0, ld_extra=0, store_win=None, store_ld=None, act=ACT_NONE):
    """One probed GEMM: x [ceil(rows / row_div), K (+ ld_extra unused columns)] at column 0, output at r4(K)."""
    n_src = -(-rows // row_div)
    w, x, b, _, _ = P.probe(kind, N, K, n_src, seed=seed + 13 * K + N)
    if ld_extra:
        x = np.concatenate([x, np.full((n_src, ld_extra), 7.5, np.float32)], 1)
    c = _r4(K)
    return [rm(x, 0, K, row_div)], [lay(w, b, 0, c, act, store="y", store_cols=store_win, store_ld=store_ld)], c + N, rows


def two_layer(kind, K, H, N, rows, probed, seed=0):
    """x -> Linear(K, H) ReLU -> Linear(H, N) with layer ``probed`` the probe and the other copying exactly; both stored."""
    if probed == 0:
        w0, x, b0, _, _ = P.probe(kind, H, K, rows, seed=seed + K + H)
        w1, b1 = P.signed_perm(N, H, seed + 3), np.zeros(N, np.float32)
    else:
        x = P.operand_like(kind, rows, K, seed + 1, "b")
        w0, b0 = P.positive_copy(H, K), np.zeros(H, np.float32)
        w1 = P.operand_like(kind, N, H, seed + 5, "a")
        b1 = P.grid_values(np.random.default_rng(seed + 9), (N,), 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)
    c_h = _r4(K)
    c_o = c_h + _ru(H, 8)
    return ([rm(x, 0)], [lay(w0, b0, 0, c_h, ACT_RELU, store="h"), lay(w1, b1, c_h, c_o, store="y")], c_o + N, rows)


def transposed_case(kind, rows=33, seed=0):
    """dgrad-style layers: W [out = 43, in = 96] used as W^T, outputs cut by n_slice into (0, 20) and (20, 96), the second
    block masked, both reading the same input."""
    W = P.operand_like(kind, 43, 96, seed + 2, "a")
    x = P.operand_like(kind, rows, 43, seed + 3, "b")
    mask = (np.random.default_rng(seed + 4).random((rows, 76)) < 0.6).astype(np.float32)
    c = _r4(43)
    return ([rm(x, 0)], [lay(W, None, 0, c, transposed=True, n_slice=(0, 20), store="a"),
                         lay(W, None, 0, c + 20, transposed=True, n_slice=(20, 96), mask=mask, store="b")], c + 96, rows)


def accumulate_case(kind, rows=33, K=20, N=80, seed=0):
    """Layer 0 is the probe; layer 1 adds a signed copy of the input onto the region layer 0 wrote (two column groups)."""
    w0, x, b0, _, _ = P.probe(kind, N, K, rows, seed=seed + 21)
    w1 = P.signed_perm(N, K, seed + 22)
    c = _ru(K, 8)
    return ([rm(x, 0)], [lay(w0, b0, 0, c, store="first"), lay(w1, None, 0, c, accumulate=True, store="y")], c + N, rows)


def fix_case(rows=33, seed=0):
    """fix_a / fix_b: column 0 += fix_a * min(fix_b, e^15) while the segment is staged, fix_b on both sides of the clamp and above
    fp32's range.  fix_a is a power of two and column 0 a small integer, so the sum is exact; a +-1 copy layer reads it out."""
    rng = np.random.default_rng(seed + 31)
    x = rng.integers(-4, 5, size=(rows, 9)).astype(np.float32)
    fb = np.array([1024.5, 3.25, 3.0e6, E15, float(np.nextafter(np.float32(E15), np.float32(np.inf))), 1.0e7, 3.0e38, np.inf],
                  np.float32)[np.arange(rows) % 8]
    fa = np.array([1.0, -1.0, 0.5], np.float32)[np.arange(rows) % 3]
    s = rm(x, 0, fix_a=fa, fix_b=fb)
    return [s], [lay(P.signed_perm(9, 9, seed + 32), None, 0, 12, store="y")], 12 + 9, rows


def level_major_case(kind, f, rows=33, seed=0):
    """Level-major input [L, rows, f] -> probe -> level-major store [L2, rows, f] and store_exp0 of output column 0."""
    L, L2 = {1: 9, 2: 5, 3: 3, 4: 3, 8: 2}[f], {1: 5, 2: 3, 3: 2, 4: 2, 8: 1}[f]
    K, N = L * f, L2 * f
    w, x, b, _, _ = P.probe(kind, N, K, rows, seed=seed + 40 + f)
    enc = np.ascontiguousarray(x.reshape(rows, L, f).transpose(1, 0, 2))
    c = _r4(K)
    return [lm(enc, 0)], [lay(w, b, 0, c, store="y", store_lm=f, store_exp0=True)], c + N, rows


# K in {1, 7, 9, 43, 70, 177}, N in {1, 3, 17, 65, 80, 112, 128, 256}, rows in {1, 15, 17, 33, 257}, row_div in {1, 5, 17, 24};
# N = 40 / 64 add the three- and four-tile column groups, K = 8 / 20 the K % 8 = 0 / 4 tails
ONE_LAYER = [(1, 1, 1, 1), (7, 3, 15, 1), (9, 17, 17, 5), (43, 65, 33, 17), (70, 80, 257, 24), (177, 112, 33, 1), (9, 128, 17, 1),
             (43, 256, 33, 5), (8, 40, 33, 24), (20, 64, 257, 17), (70, 256, 15, 1)]


def descriptor_cases():
    """{id: builder(kind) -> (segs, layers, buf_cols, n_rows)} of the descriptor-level probes."""
    cases = {}
    for K, N, rows, rd in ONE_LAYER:
        cases[f"K{K}N{N}rows{rows}div{rd}"] = (lambda kind, K=K, N=N, rows=rows, rd=rd: one_layer(kind, K, N, rows, rd))
    cases["ld_window"] = lambda kind: one_layer(kind, 43, 80, 33, ld_extra=5, store_win=(7, 75), store_ld=71)
    cases["sigmoid"] = lambda kind: one_layer(kind, 9, 17, 33, act=ACT_SIGMOID)
    cases["trunc_exp"] = lambda kind: one_layer(kind, 9, 3, 33, act=ACT_TRUNC_EXP)
    for probed in (0, 1):
        cases[f"two_layer_p{probed}"] = lambda kind, p=probed: two_layer(kind, 20, 128, 65, 257, p)
    cases["transposed_slices_mask"] = transposed_case
    cases["accumulate"] = accumulate_case
    cases["fix"] = lambda kind: fix_case()
    for f in (1, 2, 3, 4, 8):
        cases[f"level_major_f{f}"] = lambda kind, f=f: level_major_case(kind, f)
    return cases


def second_pass_cases():
    """{id: builder(kind) -> (segs, layers, buf_cols, n_rows)}: more rows than one pass of the persistent grid, the rows of the
    second pass drawn differently from the first.  Layer 0 (K = 8, N = 16) is the probe, stored.  Layer 1 (K = 4 from column
    4: K % 8 = 4) accumulates a signed copy of the input's second half onto layer 0's output; its four padded columns are
    the first four of that output region, which a wave's previous tile wrote.  "narrow": 16 waves; "wide": a 16 -> 64 -> 112
    pair of copy layers behind it, whose weights and columns leave fewer than 16 waves (decided by ``plan``, not assumed)."""
    def build(kind, wide):
        K, N, c = 8, 16, 8
        kn = [(K, N), (4, N)] + ([(N, 64), (64, 112)] if wide else [])
        cols = c + N + ((64 + 112) if wide else 0)
        first = plan(cols, kn)["rows_per_pass"]
        rows = first + 17
        w0, base, b0, _, _ = P.probe(kind, N, K, 2048, seed=61)
        xa = np.tile(base, (first // 2048, 1))
        xb = P.operand_like(kind, rows - first, K, 62, "b") * np.float32(0.5)   # second pass: other values on a finer grid
        x = np.concatenate([xa, xb], 0)
        layers = [lay(w0, b0, 0, c, store="first"), lay(P.signed_perm(N, 4, 63), None, 4, c, accumulate=True, store="y")]
        if wide:
            layers += [lay(P.signed_perm(64, N, 64), None, c, c + N, ACT_RELU), lay(P.signed_perm(112, 64, 65), None, c + N, c + N + 64, store="z")]
        return [rm(x, 0)], layers, cols, rows
    return {"narrow": lambda kind: build(kind, False), "wide": lambda kind: build(kind, True)}


# ------------------------------------------------------------------------------------------------------------ Function level
# (H, Kh, NG, C, R, S): the non-fast rgb heads.  H = 128 does not fit one chain launch (layer 1's weights alone are 96 KiB) and
# runs layer by layer; H = 96 is the widest that does and takes the layout with A2 in columns of its own.
RGB_CASES = [(32, 17, 32, 3, 7, 5), (32, 70, 64, 20, 9, 24), (128, 17, 32, 3, 7, 5), (128, 70, 64, 20, 50, 24), (96, 17, 32, 3, 11, 24),
             (64, 17, 64, 3, 8, 24)]
# (H, K0, C, rows)
SKIP_CASES = [(32, 27, 3, 33), (32, 70, 20, 257), (128, 27, 3, 33), (128, 70, 20, 257), (96, 27, 3, 257)]
# (L, F, H, NG, rows): shapes neck_supported rejects; L F not a multiple of 8 except (4, 8)
BASE_CASES = [(7, 1, 20, 64, 33), (9, 3, 32, 16, 257), (4, 8, 128, 80, 33), (5, 1, 128, 64, 257)]
# the stacks whose weights and columns fit one chain launch (128- and 256-wide hidden layers, four layers) ...
SEQ_CHAIN = [(43, 32, 5), (64, 128, 3), (27, 256, 16), (40, 128, 64, 32, 6)]
# ... and three that do not and run layer by layer (seq_mlp_supported says no)
SEQ_CASES = SEQ_CHAIN + [(70, 128, 128, 20), (27, 256, 64), (113, 128, 128, 3)]
SEQ_ROWS = 257


def skip_probe(kind, probed, H, K0, C, rows, seed, x=None):
    """Weights and input of the 3-layer skip MLP with layer ``probed`` (0, 1 or 2) the probe and the others copying exactly.
    x: the input rows to use (the rgb head's [hray of the ray | geo]) instead of drawing them.  Returns (x [rows, K0],
    [w0, b0, w1, b1, w2, b2])."""
    z = lambda n: np.zeros(n, np.float32)
    gb = lambda n, s: P.grid_values(np.random.default_rng(s), (n,), 20, P.grid_q(kind, "a") + P.grid_q(kind, "b"), nonzero=False)
    if x is None:
        x = P.operand_like(kind, rows, K0, seed, "b")
    n_copy = min(K0, H // 2)
    copy0 = P.positive_copy(H, n_copy) @ np.eye(n_copy, K0, dtype=np.float32)     # +-x_j of the first n_copy inputs
    pass1 = np.concatenate([np.abs(P.signed_perm(H, H, seed + 1)), np.zeros((H, K0), np.float32)], 1)   # a2 = a permutation of a1
    w0, b0, w1, b1, w2, b2 = copy0, z(H), pass1, z(H), P.signed_perm(C, H, seed + 2), z(C)
    if probed == 0:
        w0, b0 = P.operand_like(kind, H, K0, seed + 4, "a"), gb(H, seed + 3)
    elif probed == 1:
        if kind != "hl":   # a1 and the skip input share one row of layer 1: at most 3 + 3 non-zeros
            x = x.copy()
            x[np.cumsum(x != 0, 1) > 3] = 0.0
        w1 = np.concatenate([P.operand_like(kind, H, H, seed + 5, "a"), P.operand_like(kind, H, K0, seed + 6, "a")], 1)
        b1 = gb(H, seed + 7)
    else:
        w2, b2 = P.operand_like(kind, C, H, seed + 8, "a"), gb(C, seed + 9)
    return x, [w0, b0, w1, b1, w2, b2]


def rgb_rows(kind, R, S, Kh, NG, seed):
    """(hray [R, Kh], geo [R S, NG], the concatenated rows [R S, Kh + NG]) with the probe's activation distribution."""
    xr = P.operand_like(kind, R, Kh, seed + 1, "b")
    xg = P.operand_like(kind, R * S, NG, seed + 2, "b")
    if kind != "hl":   # at most 3 non-zeros per row over both parts (layer 1 adds a1's)
        xr = xr.copy(); xr[np.cumsum(xr != 0, 1) > 1] = 0.0
        xg = xg.copy(); xg[np.cumsum(xg != 0, 1) > 2] = 0.0
    return xr, xg, np.concatenate([np.repeat(xr, S, 0), xg], 1)


def skip_ref(x, ws):
    """fp64 forward of the skip MLP through P.mlp_ref (which asserts every layer inside the exact budget): a1, a2, z (pre-activation
    of the output layer), and the pieces P.mlp_ref_bwd needs per layer."""
    w0, b0, w1, b1, w2, b2 = ws
    hs0, pre0 = P.mlp_ref(x, [w0], [b0], [True])
    c = np.concatenate([hs0[1], np.asarray(x, np.float64)], 1)
    hs1, pre1 = P.mlp_ref(c, [w1], [b1], [True])
    hs2, pre2 = P.mlp_ref(hs1[1], [w2], [b2], [False])
    return {"a1": hs0[1], "a2": hs1[1], "z": pre2[0], "c": c, "pre0": pre0[0], "pre1": pre1[0]}


def skip_ref_bwd(x, ws, ref, g):
    """fp64 backward of the skip MLP WITHOUT a final activation for the output gradient g: {"dx", "dpre1", "dpre0"} and ``ok``,
    the rows on which every data-gradient GEMM -- dA2 = g W2, d[A1 | x] = dPre1 W1, dA1 W0 and the sum of the two gradients of
    the skip input -- stays inside the exact budget (whole rows: an inexact entry may feed every entry of its row)."""
    w0, w1, w2 = (np.asarray(ws[i], np.float64) for i in (0, 2, 4))
    H = w0.shape[0]
    g = np.asarray(g, np.float64)
    dpre1 = (g @ w2) * (ref["pre1"] > 0)
    dc = dpre1 @ w1
    dpre0 = dc[:, :H] * (ref["pre0"] > 0)
    d0 = dpre0 @ w0
    q = max(P.grid_of(dpre0) + P.grid_of(w0), P.grid_of(dc[:, H:]))
    u0 = P.abs_units(w0.T, dpre0, None, q) + np.abs(dc[:, H:]) * 2.0 ** q
    ok1 = (P.units(w2.T, g) < P.BUDGET).all(1)               # rows whose dPre1 is exact
    ok0 = ok1 & (P.units(w1.T, dpre1) < P.BUDGET).all(1)     # ... whose dPre0 is
    ok = ok0 & (u0 < P.BUDGET).all(1)
    out = {"dx": d0 + dc[:, H:], "dpre1": dpre1, "dpre0": dpre0, "ok": ok}
    # weight gradients, marked as P.mlp_ref_bwd marks them: the entry's own row sum inside the budget and fed by exact rows only
    for i, (d, h, okd) in enumerate(((dpre0, np.asarray(x, np.float64), ok0), (dpre1, ref["c"], ok1), (g, ref["a2"], np.ones_like(ok)))):
        bad = np.where(okd[:, None], 0.0, np.abs(d))
        uw = P.units(d.T, h.T).T
        out[f"dW{i}"] = (d.T @ h, (uw < P.BUDGET) & ((bad.T @ np.abs(h)) == 0))
        ub = P.plane_mag(d).sum(0) * 2.0 ** P.grid_of(d)
        out[f"db{i}"] = (d.sum(0), (ub < P.BUDGET) & (bad.sum(0) == 0))
    return out
