"""The path functions of emernerf_amd/fused.py (which kernels a head's forward and backward run; the table in its module docstring)
on the host: the shipped shapes, every flag combination the GPU tests use, and the edges of each predicate.  They read the module
flags and the library's host-only queries, so no GPU is needed (as tests/test_host_cpu.py::test_slice_plan_host_logic)."""
import types

import pytest

from tests._chain_probe import BASE_CASES, RGB_CASES, SEQ_CHAIN, SKIP_CASES
from tests._fused_paths import DEFAULT_FLAGS

M = 1 << 20
# the five modes of tests/test_fused_gpu.py::test_rgb_head -> (flags, the rgb head's path, what rgb_recompute reports)
RGB_MODES = {"all": (dict(RGB_RECOMPUTE=1), "recompute_a1a2", 1),
             "all_a2": (dict(RGB_RECOMPUTE=2), "recompute_a2", 2),
             "all_stored": ({}, "fused", 0),
             "w2_only": (dict(FUSED_RGB_WGRAD=False), "w2_in_kernel", 0),
             "False": (dict(FUSED_WGRAD=False, FUSED_RGB_WGRAD=False), "streamed", 0)}
FLOW = (40, 64, 64, 6)          # on the level-major xyzt encoding, L 10, F 4
FEATURE = (64, 64, 64, 64)      # row-major


def _ws(dims):
    """Stand-ins for Linear weights: the path functions read their shapes only."""
    return [types.SimpleNamespace(shape=(dims[i + 1], dims[i])) for i in range(len(dims) - 1)]


@pytest.fixture
def fused(hip_lib, monkeypatch):
    from emernerf_amd import fused as F
    for k, v in DEFAULT_FLAGS.items():
        monkeypatch.setattr(F, k, v)
    return F


def _set(monkeypatch, F, **kw):
    for k, v in kw.items():
        monkeypatch.setattr(F, k, v)


def _rgb(F, need_grad=True, R=8192, S=128, Kh=49, H=64, NG=64, C=3, ld=64, ptr=0):
    return F.rgb_head_path(R, S, Kh, H, NG, C, ld, ptr, need_grad)


def test_shipped_shapes_with_the_default_flags(fused):
    F = fused
    assert [F.neck_path(16, 2, M, 128, g) for g in (True, False)] == ["fused", "streamed"]
    assert [F.neck_path(10, 4, M, 64, g) for g in (True, False)] == ["fused", "streamed"]
    assert [F.density_mlp_path(8, 1, M, 64, g) for g in (True, False)] == ["fused", "neck_streamed"]
    assert [_rgb(F, g) for g in (True, False)] == ["fused", "streamed"]
    assert [F.seq_mlp_path(_ws(FLOW), 4, M, g) for g in (True, False)] == ["fused", "streamed"]
    assert [F.seq_mlp_path(_ws(FEATURE), 0, M, g) for g in (True, False)] == ["fused", "streamed"]
    assert F.seq_mlp_path(_ws(FLOW), 4, M, True, hidden_biases=False) == "streamed"   # the recomputation needs the hidden biases
    assert [F.skip_mlp3_path(8192, 43, 64, 3, g) for g in (True, False)] == ["ray", "ray"]


@pytest.mark.parametrize("mode", list(RGB_MODES))
def test_rgb_modes_and_rgb_recompute(fused, monkeypatch, mode):
    F = fused
    flags, path, rec = RGB_MODES[mode]
    _set(monkeypatch, F, **flags)
    assert _rgb(F) == path
    assert _rgb(F, need_grad=False) == "streamed"   # inference: nothing stored, no backward chosen
    assert F.rgb_recompute(8192, 128) == rec == {"recompute_a1a2": 1, "recompute_a2": 2}.get(_rgb(F), 0)
    # the predicate's edges: S = 24 is no multiple of 16, a pitch or an address off the 16-byte grid -> the chain kernel
    assert _rgb(F, S=24) == _rgb(F, ld=66) == _rgb(F, ptr=4) == _rgb(F, Kh=65) == "chain"
    assert F.rgb_recompute(8192, 24) == 0 and F.rgb_recompute(0, 128) == 0
    assert _rgb(F, S=16, ld=128, ptr=16) == path


def test_fused_wgrad_off(fused, monkeypatch):
    F = fused
    _set(monkeypatch, F, FUSED_WGRAD=False)
    assert F.neck_path(16, 2, M, 128, True) == F.neck_path(10, 4, M, 64, True) == "streamed"
    assert F.density_mlp_path(8, 1, M, 64, True) == "neck_streamed"
    assert F.seq_mlp_path(_ws(FLOW), 4, M, True) == F.seq_mlp_path(_ws(FEATURE), 0, M, True) == "streamed"
    assert not F.rmlp_bwd_fused_supported(_ws(FLOW), 40, 4, M)


@pytest.mark.parametrize("flags,flow,feature", [({}, "fused", "fused"), (dict(FUSED_RMLP_WGRAD=False), "streamed", "streamed"),
                                                (dict(FUSED_RMLP_WIDE=False), "fused", "streamed")])
def test_plain_stacks_and_rmlp_bwd_fused_supported(fused, monkeypatch, flags, flow, feature):
    F = fused
    _set(monkeypatch, F, **flags)
    assert F.seq_mlp_path(_ws(FLOW), 4, M, True) == flow and F.seq_mlp_path(_ws(FLOW[:1] + FLOW[2:]), 4, M, True) == flow
    assert F.seq_mlp_path(_ws(FEATURE), 0, M, True) == feature
    assert F.rmlp_bwd_fused_supported(_ws(FLOW), 40, 4, M) == (flow == "fused")
    assert F.rmlp_bwd_fused_supported(_ws(FEATURE), 64, 0, M) == (feature == "fused")
    assert F.seq_mlp_path(_ws(FLOW), 4, 1 << 25, True) == "streamed"   # level-major: 32-bit lane offsets end at n k0 = 2^30


def test_edges(fused):
    F = fused
    # neck: n L F at 2^30 (32-bit lane offsets of the fused backward)
    assert F.neck_path(16, 2, (1 << 25) - 1, 128, True) == "fused" and F.neck_path(16, 2, 1 << 25, 128, True) == "streamed"
    # density: the fused backward holds L F <= 16 inputs
    assert F.density_mlp_path(8, 2, M, 64, True) == "fused" and F.density_mlp_path(12, 2, M, 64, True) == "neck_streamed"
    # skip head: one ray_wgrad launch up to 65536 rows
    assert F.skip_mlp3_path(65536, 43, 64, 3) == "ray" and F.skip_mlp3_path(65537, 43, 64, 3) == "ray_streamed"
    assert F.skip_mlp3_path(33, 64, 64, 16) == "ray" and F.skip_mlp3_path(33, 65, 64, 3) == F.skip_mlp3_path(33, 43, 64, 17) == "chain"


def test_chain_shapes(fused):
    F = fused
    H, Kh, NG, C, R, S = RGB_CASES[0]
    assert F.rgb_head_supported(H, Kh, NG, C) and _rgb(F, R=R, S=S, Kh=Kh, H=H, NG=NG, C=C, ld=NG) == "chain"
    H, K0, C, rows = SKIP_CASES[0]
    assert F.skip_mlp3_supported(H, K0, C) and F.skip_mlp3_path(rows, K0, H, C) == "chain"
    L, Fe, H, NG, rows = BASE_CASES[0]
    assert F.base_mlp_supported(L * Fe, H, NG) and F.density_mlp_supported(L * Fe, H)
    assert [F.density_mlp_path(L, Fe, rows, H, g) for g in (True, False)] == ["chain", "chain"]
    ws = _ws(SEQ_CHAIN[0])
    assert F.seq_mlp_supported(ws) and [F.seq_mlp_path(ws, 0, 257, g) for g in (True, False)] == ["chain", "chain"]
