"""The forward and data-gradient entry points of csrc/mlp_fused.hip called directly (emer_neck_fwd / _bwd, emer_rgb_head_fwd / _bwd,
emer_field_fwd, emer_rmlp_fwd / _bwd) on seeded CPU-generated inputs, with any optional pointer null: emernerf_amd.fused passes the
combinations the training step needs, so only direct calls reach the others.  Output buffers start at 7.5, so a store that should not
happen shows; with `guard` they are followed by sentinel rows, so a store past the end shows too.  Shared by tests/test_fused_gpu.py,
tests/test_field_exact_gpu.py (which supplies its own arrays to rgb_case) and tools/head_entry_digests.py; `call` is emernerf_amd._lib.call or a stand-in with
its signature (the tool times two builds of the library in one process), `o` the output buffers of an earlier call to be used again."""
import torch

from emernerf_amd import _lib
from emernerf_amd.ops import _ptr, _stream

DEV = torch.device("cuda:0")


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _rnd(g, *shape, k=1.0):
    return (torch.randn(*shape, generator=g) * k).to(DEV)


GUARD = -3.25   # the fill of the sentinel rows


def buf(*shape, guard=0):
    """An output buffer filled with 7.5; guard > 0: the first rows of a taller allocation whose `guard` further rows hold GUARD."""
    if not guard:
        return torch.full(shape, 7.5, device=DEV, dtype=torch.float32)
    full = torch.full((shape[0] + guard,) + tuple(shape[1:]), 7.5, device=DEV, dtype=torch.float32)
    full[shape[0]:] = GUARD
    return full[:shape[0]]


def guard_rows(t):
    """The sentinel rows behind a buffer made by buf(..., guard=n)."""
    return t._base[t.shape[0]:]


def _dev(x):
    return torch.as_tensor(x, dtype=torch.float32).to(DEV).contiguous()


def _pick(tensors, null):
    return {k: (None if k in null else v) for k, v in tensors.items()}


# ---------------------------------------------------------------------------------------------------------------- neck
def neck_case(L, F, n_out, N):
    g, K0 = _gen(L, F, n_out, N), L * F
    return dict(L=L, F=F, n_out=n_out, N=N, enc=_rnd(g, L, N, F, k=0.5), w0=_rnd(g, 64, K0, k=K0 ** -0.5), b0=_rnd(g, 64, k=0.1),
                w1=_rnd(g, n_out, 64, k=0.125), b1=_rnd(g, n_out, k=0.1), d0=_rnd(g, N, 64), d1=_rnd(g, N, 64), ddens=_rnd(g, N))


def neck_fwd(c, null=(), call=_lib.call, o=None):
    """Optional: h1; dens when n_out > 1.  Returns the output buffers (None where null or not an output of this n_out)."""
    N, n_out = c["N"], c["n_out"]
    o = o or _pick(dict(h1=buf(N, 64), out0=buf(N, 64) if n_out > 1 else None, out1=buf(N, 64) if n_out == 128 else None, dens=buf(N)), null)
    call("emer_neck_fwd", _ptr(c["enc"]), c["L"], c["F"], N, _ptr(c["w0"]), _ptr(c["b0"]), _ptr(c["w1"]), _ptr(c["b1"]), n_out, _ptr(o["h1"]),
         _ptr(o["out0"]), _ptr(o["out1"]), _ptr(o["dens"]), _stream(c["enc"]))
    return o


def neck_bwd(c, fwd, null=(), call=_lib.call, o=None):
    """fwd: neck_fwd(c) with every pointer given.  Optional: d0, d1 (n_out == 128), ddens, dcol0; n_out == 1 takes ddens only."""
    N, n_out = c["N"], c["n_out"]
    if n_out == 1:
        g = dict(d0=None, d1=None, ddens=c["ddens"])
        o = o or dict(dpre1=buf(N), dcol0=None, dpre0=buf(N, 64), denc=buf(c["L"], N, c["F"]))
    else:
        g = _pick(dict(d0=c["d0"], d1=c["d1"] if n_out == 128 else None, ddens=c["ddens"]), null)
        o = o or _pick(dict(dpre1=None, dcol0=buf(N), dpre0=buf(N, 64), denc=buf(c["L"], N, c["F"])), null)
    call("emer_neck_bwd", _ptr(g["d0"]), _ptr(g["d1"]), _ptr(g["ddens"]), _ptr(fwd["dens"]), _ptr(fwd["h1"]), c["L"], c["F"], N, _ptr(c["w0"]),
         _ptr(c["w1"]), n_out, _ptr(o["dpre1"]), _ptr(o["dcol0"]), _ptr(o["dpre0"]), _ptr(o["denc"]), _stream(c["enc"]))
    return o


# ------------------------------------------------------------------------------------------------ rgb head, field forward
RB_JUNK = 977.0    # the fill of the pad columns of rb when ld_rb > 128
W_PAD_ROWS = 2     # rows of junk behind the head's w0 / w1 with pad_w (a view cut at a wrong column offset then stays inside the allocation)


def rgb_case(R, S, Kh=49, L=0, F=0, ld_rb=128, arrays=None, pad_w=False):
    """The rgb head on R rays of S samples; with L, F also the neck in front of it (emer_field_fwd's input).

    ld_rb: leading dimension of rb [R][ld_rb] = [rb0 | rb1 | pad columns holding RB_JUNK].  arrays: caller-supplied values (numpy or
    torch, any of geo, rb0, rb1 [R][64], w0, w1, w2, b2, enc, nw0, nb0, nw1, nb1) that replace the seeded ones; what is supplied is not
    drawn, so the other seeded tensors then differ from those of a call without arrays.  pad_w: w0 / w1 are the first 64 rows of
    matrices with W_PAD_ROWS more rows of junk."""
    g, N, given = _gen(R, S, Kh, L, F), R * S, dict(arrays or {})
    assert ld_rb >= 128 and ld_rb % 4 == 0

    def pick(name, *shape, k=1.0):
        return _dev(given.pop(name)) if name in given else _rnd(g, *shape, k=k)

    def tall(w):
        return torch.cat([w, torch.full((W_PAD_ROWS, w.shape[1]), 61.0, device=DEV)])[:64] if pad_w else w

    geo = pick("geo", N, 64)
    if "rb0" in given or "rb1" in given:
        rb = torch.cat([_dev(given.pop("rb0")), _dev(given.pop("rb1"))], 1)
    else:
        rb = _rnd(g, R, 128, k=0.5)
    assert rb.shape == (R, 128)
    if ld_rb > 128:
        rb = torch.cat([rb, torch.full((R, ld_rb - 128), RB_JUNK, device=DEV)], 1)
    c = dict(R=R, S=S, Kh=Kh, N=N, ld_rb=ld_rb, geo=geo, rb=rb, w0=tall(pick("w0", 64, Kh + 64, k=0.1)), w1=tall(pick("w1", 64, 128 + Kh, k=0.1)),
             w2=pick("w2", 3, 64, k=0.125), b2=pick("b2", 3, k=0.1), dout=_rnd(g, N, 3))
    if L:
        K0 = L * F
        c.update(L=L, F=F, enc=pick("enc", L, N, F, k=0.5), nw0=pick("nw0", 64, K0, k=K0 ** -0.5), nb0=pick("nb0", 64, k=0.1),
                 nw1=pick("nw1", 64, 64, k=0.125), nb1=pick("nb1", 64, k=0.1))
        assert c["enc"].shape == (L, N, F) and c["nw0"].shape == (64, K0)
    assert not given, f"unknown arrays: {sorted(given)}"
    assert c["w0"].shape == (64, Kh + 64) and c["w1"].shape == (64, 128 + Kh) and c["w0"].is_contiguous() and c["w1"].is_contiguous()
    return c


def neck_of(c):
    """The neck in front of the rgb head of rgb_case(..., L, F) as a case of neck_fwd (n_out = 64)."""
    return dict(L=c["L"], F=c["F"], n_out=64, N=c["N"], enc=c["enc"], w0=c["nw0"], b0=c["nb0"], w1=c["nw1"], b1=c["nb1"])


def rgb_head_fwd(c, null=(), geo=None, call=_lib.call, o=None, guard=0):
    """Optional: a2, or a1 and a2.  guard: sentinel rows behind every output buffer (buf)."""
    geo = c["geo"] if geo is None else geo
    o = o or _pick(dict(a1=buf(c["N"], 64, guard=guard), a2=buf(c["N"], 64, guard=guard), out=buf(c["N"], 3, guard=guard)), null)
    call("emer_rgb_head_fwd", _ptr(geo), 64, _ptr(c["rb"]), _ptr(c["rb"][:, 64:]), c.get("ld_rb", 128), c["R"], c["S"], c["Kh"], _ptr(c["w0"]),
         _ptr(c["w1"]), _ptr(c["w2"]), _ptr(c["b2"]), _ptr(o["a1"]), _ptr(o["a2"]), _ptr(o["out"]), _stream(geo))
    return o


def field_fwd(c, null=(), call=_lib.call, o=None, guard=0):
    """Optional: a2, or a1 and a2.  guard: sentinel rows behind every output buffer (buf)."""
    N = c["N"]
    o = o or _pick(dict(geo=buf(N, 64, guard=guard), dens=buf(N, guard=guard), a1=buf(N, 64, guard=guard), a2=buf(N, 64, guard=guard),
                        out=buf(N, 3, guard=guard)), null)
    call("emer_field_fwd", _ptr(c["enc"]), c["L"], c["F"], c["R"], c["S"], _ptr(c["nw0"]), _ptr(c["nb0"]), _ptr(c["nw1"]), _ptr(c["nb1"]),
         _ptr(c["rb"]), _ptr(c["rb"][:, 64:]), c.get("ld_rb", 128), c["Kh"], _ptr(c["w0"]), _ptr(c["w1"]), _ptr(c["w2"]), _ptr(c["b2"]), _ptr(o["geo"]),
         _ptr(o["dens"]), _ptr(o["a1"]), _ptr(o["a2"]), _ptr(o["out"]), _stream(c["enc"]))
    return o


def rgb_head_bwd(c, fwd, with_dw2, call=_lib.call, o=None):
    """fwd: rgb_head_fwd(c) with every pointer given.  dw2 / db2 are accumulated (+=) on top of the 7.5 they start with."""
    N, R = c["N"], c["R"]
    o = o or dict(dpre2=buf(N, 3), dpre1=buf(N, 64), dpre0=buf(N, 64), dgeo=buf(N, 64), s1=buf(R, 64), s0=buf(R, 64))
    ws = dw2 = db2 = None
    if with_dw2:
        ws, dw2, db2 = buf(int(_lib.load().emer_rgb_head_bwd_workspace(R))), buf(3, 64), buf(3)
        o.update(dw2=dw2, db2=db2)
    call("emer_rgb_head_bwd", _ptr(c["dout"]), _ptr(fwd["out"]), _ptr(fwd["a1"]), _ptr(fwd["a2"]), R, c["S"], c["Kh"], _ptr(c["w0"]), _ptr(c["w1"]),
         _ptr(c["w2"]), _ptr(o["dpre2"]), _ptr(o["dpre1"]), _ptr(o["dpre0"]), _ptr(o["dgeo"]), _ptr(o["s1"]), _ptr(o["s0"]), _ptr(ws), _ptr(dw2), 64,
         _ptr(db2), _stream(c["dout"]))
    return o


# --------------------------------------------------------------------------------------------------------- plain heads
def rmlp_case(n_layers, level_major, k0, n_out, N, sigmoid=False):
    """Input: row-major [N][k0] or level-major [k0 / 4][N][4]."""
    g = _gen(n_layers, level_major, k0, n_out, N)
    x = _rnd(g, k0 // 4, N, 4, k=0.5) if level_major else _rnd(g, N, k0, k=0.5)
    c = dict(n_layers=n_layers, lm=bool(level_major), k0=k0, n_out=n_out, N=N, x=x, act=_lib.ACT_SIGMOID if sigmoid else _lib.ACT_NONE,
             w0=_rnd(g, 64, k0, k=k0 ** -0.5), b0=_rnd(g, 64, k=0.1), dlast=_rnd(g, N, n_out))
    if n_layers == 3:
        c.update(w1=_rnd(g, 64, 64, k=0.125), b1=_rnd(g, 64, k=0.1), w2=_rnd(g, n_out, 64, k=0.125), b2=_rnd(g, n_out, k=0.1))
    else:   # two layers: the output layer goes in as w1 / b1
        c.update(w1=_rnd(g, n_out, 64, k=0.125), b1=_rnd(g, n_out, k=0.1), w2=None, b2=None)
    return c


def _rmlp_layout(c):
    return (c["k0"] // 4, 4, 0) if c["lm"] else (0, 0, c["k0"])   # n_levels, n_feat, leading dimension of x / dx


def rmlp_fwd(c, null=(), call=_lib.call, o=None):
    """Optional: h1, h2 (three layers)."""
    N, L, F, ld = c["N"], *_rmlp_layout(c)
    o = o or _pick(dict(h1=buf(N, 64), h2=buf(N, 64) if c["n_layers"] == 3 else None, out=buf(N, c["n_out"])), null)
    call("emer_rmlp_fwd", _ptr(c["x"]), ld, L, F, c["k0"], N, c["n_layers"], _ptr(c["w0"]), _ptr(c["b0"]), _ptr(c["w1"]), _ptr(c["b1"]), _ptr(c["w2"]),
         _ptr(c["b2"]), c["n_out"], c["act"], _ptr(o["h1"]), _ptr(o["h2"]), _ptr(o["out"]), c["n_out"], _stream(c["x"]))
    return o


def rmlp_bwd(c, fwd, null=(), call=_lib.call, o=None):
    """fwd: rmlp_fwd(c) with every pointer given.  Optional: dx."""
    N, L, F, ld = c["N"], *_rmlp_layout(c)
    o = o or _pick(dict(dpre1=buf(N, 64) if c["n_layers"] == 3 else None, dpre0=buf(N, 64), dx=torch.full_like(c["x"], 7.5)), null)
    call("emer_rmlp_bwd", _ptr(c["dlast"]), c["n_out"], _ptr(fwd["h1"]), _ptr(fwd["h2"]), L, F, c["k0"], N, c["n_layers"], _ptr(c["w0"]), _ptr(c["w1"]),
         _ptr(c["w2"]), c["n_out"], _ptr(o["dpre1"]), _ptr(o["dpre0"]), _ptr(o["dx"]), ld, _stream(c["x"]))
    return o
