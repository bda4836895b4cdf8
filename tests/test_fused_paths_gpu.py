"""Every row of the path table of emernerf_amd/fused.py (its module docstring) on the GPU: one forward and one backward per case of
tests/_fused_paths.py, at the smallest shape that still has two tiles or two rays.  Checked: the path the Function recorded
(``out.grad_fn.path``) and the names passed to ``_lib.call`` during each pass.

EXPECTED was recorded with tools/head_digests.py --launches --tree on the commit BEFORE the Functions were rewritten around
``ctx.path`` (profiles/fused_paths_ab.json), not taken from the code under test: the rewrite must launch what its parent launched."""
import pytest
import torch

from tests import _fused_paths as T

pytestmark = pytest.mark.gpu

_RGB_FWD = ["emer_ray_pre_fwd", "emer_rgb_head_fwd"]
_TAIL = ["emer_ray_wgrad", "emer_ray_pre_bwd"]
_W = "emer_wgrad_segmented"
_SKY_FWD = ["emer_ray_pre_fwd", "emer_ray_head_fwd"]
EXPECTED = {   # case: (forward, backward)
    "rgb fused": (_RGB_FWD, ["emer_rgb_head_bwd_fused"] + _TAIL),
    "rgb recompute_a1a2": (_RGB_FWD, ["emer_rgb_head_bwd_recompute"] + _TAIL),
    "rgb recompute_a2": (_RGB_FWD, ["emer_rgb_head_bwd_recompute"] + _TAIL),
    "rgb w2_in_kernel": (_RGB_FWD, ["emer_rgb_head_bwd", _W, _W] + _TAIL),
    "rgb streamed": (_RGB_FWD, ["emer_rgb_head_bwd", _W, _W, _W] + _TAIL),
    "rgb chain": (["emer_mlp_chain"], ["emer_mlp_chain", _W, _W, _W]),
    "neck 4x2 64 fused": (["emer_neck_fwd"], ["emer_neck_bwd_fused"]),
    "neck 4x2 64 streamed": (["emer_neck_fwd"], ["emer_neck_bwd", _W, _W]),
    "neck 10x4 128 fused": (["emer_neck_fwd"], ["emer_neck_bwd_fused"]),
    "neck 10x4 128 streamed": (["emer_neck_fwd"], ["emer_neck_bwd", _W, _W, _W]),
    "density 8x1 fused": (["emer_neck_fwd"], ["emer_density_bwd_fused"]),
    "density 8x1 neck_streamed": (["emer_neck_fwd"], ["emer_neck_bwd", _W, _W]),
    "density 12x2 neck_streamed": (["emer_neck_fwd"], ["emer_neck_bwd", _W, _W]),
    "density chain": (["emer_mlp_chain"], ["emer_mlp_chain", _W, _W]),
    "base chain": (["emer_mlp_chain"], ["emer_mlp_chain", _W, _W]),
    "skip ray": (_SKY_FWD, ["emer_ray_head_bwd", "emer_ray_pre_bwd", "emer_ray_wgrad"]),
    "skip ray_streamed": (_SKY_FWD, ["emer_ray_head_bwd", "emer_ray_pre_bwd", _W, _W, _W]),
    "skip chain": (["emer_mlp_chain"], ["emer_mlp_chain", _W, _W, _W]),
    "seq 40-64-64-6 fused": (["emer_rmlp_fwd"], ["emer_rmlp_bwd_fused"]),
    "seq 40-64-64-6 streamed": (["emer_rmlp_fwd"], ["emer_rmlp_bwd", _W, _W, _W]),
    "seq_lm 10x4 fused": (["emer_rmlp_fwd"], ["emer_rmlp_bwd_fused"]),
    "seq_lm 10x4 streamed": (["emer_rmlp_fwd"], ["emer_rmlp_bwd", _W, _W, _W]),
    "seq 64-64-64-64 fused": (["emer_rmlp_fwd"], ["emer_rmlp_bwd_fused"]),
    "seq 64-64-64-64 streamed": (["emer_rmlp_fwd"], ["emer_rmlp_bwd", _W, _W, _W]),
    "seq chain": (["emer_mlp_chain"], ["emer_mlp_chain", _W, _W]),
}


def _recorded(monkeypatch, case_id, before_backward=None):
    """(outputs, leaves, names of the forward, names of the backward) of one run of the case with _lib.call recorded."""
    from emernerf_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    outs, leaves = T.run_case(case_id, torch.device("cuda:0"), names, before_backward)
    torch.cuda.synchronize()
    monkeypatch.setattr(_lib, "call", real)
    cut = names.index(T.BACKWARD)
    return outs, leaves, names[:cut], names[cut + 1:]


def test_the_table_is_covered():
    assert set(EXPECTED) == set(T.CASES)
    paths = {(head, path) for head, path, _, _ in T.CASES.values()}
    assert paths == {("neck", "fused"), ("neck", "streamed"), ("density_mlp", "fused"), ("density_mlp", "neck_streamed"), ("density_mlp", "chain"),
                     ("base_mlp", "chain"), ("rgb_head", "fused"), ("rgb_head", "recompute_a1a2"), ("rgb_head", "recompute_a2"),
                     ("rgb_head", "w2_in_kernel"), ("rgb_head", "streamed"), ("rgb_head", "chain"), ("skip_mlp3", "ray"),
                     ("skip_mlp3", "ray_streamed"), ("skip_mlp3", "chain"), ("seq_mlp", "fused"), ("seq_mlp", "streamed"), ("seq_mlp", "chain"),
                     ("seq_mlp_lm", "fused"), ("seq_mlp_lm", "streamed")}


@pytest.mark.parametrize("case_id", list(T.CASES))
def test_path_and_library_calls(hip_lib, monkeypatch, case_id):
    outs, leaves, fwd, bwd = _recorded(monkeypatch, case_id)
    assert outs[0].grad_fn.path == T.CASES[case_id][1]
    assert (fwd, bwd) == EXPECTED[case_id]
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)


def test_the_forward_path_holds_when_a_flag_changes_before_the_backward(hip_lib, monkeypatch):
    """The one intended difference from the code before ``ctx.path``, in the harmless direction: the forward ran with FUSED_RGB_WGRAD
    off and stored a1 / a2; the flag is on when the backward runs.  The backward is still the one the forward chose."""
    from emernerf_amd import fused

    def switch_on():
        fused.FUSED_RGB_WGRAD = True   # (T.flags restores the flag when the case ends)
    outs, leaves, fwd, bwd = _recorded(monkeypatch, "rgb w2_in_kernel", before_backward=switch_on)
    assert outs[0].grad_fn.path == "w2_in_kernel" and (fwd, bwd) == EXPECTED["rgb w2_in_kernel"]
    outs0, leaves0, _, _ = _recorded(monkeypatch, "rgb w2_in_kernel")
    assert torch.equal(outs[0], outs0[0])
    for i, (a, b) in enumerate(zip(leaves, leaves0)):
        assert torch.equal(a.grad, b.grad), f"gradient of leaf {i}"
