"""K-step TRAINING parity (second half of BASELINE.json's metric: "PSNR vs ref").

Every other gradient test compares ONE step.  Here the HIP trainer and the CPU oracle train from identical parameters for K
optimizer steps on rays coloured by a fixed synthetic ground-truth field -- proposal schedule (both step types), LR warm-up,
Adam with eps = 1e-15 and the never-unscaled x1024 loss scale, in-place table gradients, hipGraph replay -- and must stay
together: per-step loss, parameters after K steps, and the PSNR of an evaluation render of each against the ground truth
(datasets/metrics.py:31-46; train_emernerf.py:634-745).  The oracle side uses torch's own Adam / ChainedScheduler exactly as
builders.py:50-89,114-142 constructs them.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_CACHE = {}


def _run(kind, K, use_graph, table_init):
    from oracle.train_parity import cotrain
    key = (kind, K, use_graph, table_init)
    if key not in _CACHE:
        # static / dynamic: 512 rays x 64 samples (proposal rounds 64 + 32); flow / feature (seven xyzt evaluations per sample on the
        # CPU oracle): 256 rays x 32 samples (proposal rounds 32 + 16)
        shape = dict(rays=256, samples=32, prop_samples=(32, 16)) if kind in ("flow", "feature") else dict(rays=512, samples=64, prop_samples=(64, 32))
        _CACHE[key] = cotrain(kind, torch.device("cuda:0"), K=K, num_iters=200, table_init=table_init, use_graph=use_graph, **shape)
    return _CACHE[key]


@pytest.mark.parametrize("kind,K,use_graph,table_init", [("static", 30, False, 0.3), ("static", 30, True, 0.3), ("static", 30, False, None),
                                                         ("dynamic", 10, False, 0.3), ("flow", 8, False, 0.3), ("flow", 8, True, 0.3),
                                                         ("feature", 8, False, 0.3)])
def test_k_step_training_stays_with_the_oracle(hip_lib, oracle, kind, K, use_graph, table_init):
    """K optimizer steps of the HIP trainer and of the oracle from identical parameters, num_iters = 200 (so that the K steps cross
    the LR warm-up: 0.01 -> 1 over 20 steps) and a proposal schedule that reaches its one-in-six steady state inside K.
    ``table_init`` None = tcnn's +-1e-4 initialisation (the reference's step 0), 0.3 = spatially varying tables.  flow / feature =
    BASELINE configs[3] / [4]: flow-warped temporal aggregation with the noise replayed, flow-cycle loss (train_emernerf.py:700-716,
    radiance_field.py:553-620), feature head + learnable PE with the feature L2 loss."""
    r = _run(kind, K, use_graph, table_init)
    assert r["launch_mode"] == ("hipgraph" if use_graph else "eager"), "graph capture fell back to eager launches"
    assert any(r["prop_flags"]) and not all(r["prop_flags"]), "K steps must contain both step types"
    hl, rl = np.array(r["hip_losses"]), np.array(r["ref_losses"])
    assert np.isfinite(hl).all() and np.isfinite(rl).all()
    assert hl[-3:].mean() < hl[:3].mean(), "training must reduce the loss"
    print(f"\n[{kind} K={K} graph={use_graph} init={table_init}] loss {hl[0]:.5f} -> {hl[-1]:.5f}; max rel loss diff {r['loss_max_rel_diff']:.2e}; "
          f"PSNR vs GT hip {r['hip_psnr_vs_gt_db']:.4f} dB / oracle {r['ref_psnr_vs_gt_db']:.4f} dB; travel {r['travel']:.3e}, "
          f"param l2 diff {r['param_l2_diff']:.3e} (without the {r['n_sign_flipped']} sign-flipped table entries of {r['n_table_entries']}: "
          f"{r['param_l2_diff_excl']:.3e}), max abs {r['param_max_abs_diff']:.3e}")
    # (1) the loss trajectory, step by step
    # (measured on MI355X: 1e-7 .. 3e-6)
    assert r["loss_max_rel_diff"] <= 5e-5, f"per-step loss differs by {r['loss_max_rel_diff']:.3e} relative"
    # (2) PSNR against the ground truth after K steps: both paths within 0.005 dB of each other (measured: equal to 4 decimals)
    assert abs(r["hip_psnr_vs_gt_db"] - r["ref_psnr_vs_gt_db"]) <= 0.005
    # (3) the parameters after K steps: the two trajectories' distance is a small fraction of the distance travelled
    # (measured: 6e-5 with +-0.3 tables, 2e-4 dynamic).  [r6] ONE bound for every case.  From tcnn's +-1e-4 initialisation most table
    # entries' gradients are rounding-sized and Adam's first steps are sign-sized, so an entry whose gradient changes sign between
    # the two sides ends a whole step away: those entries are identified (further apart than half of the smallest step of the
    # schedule, oracle/train_parity.py), COUNTED and bounded in number, and everything else keeps the bound of the other cases --
    # round 5 had widened the bound 3x for this case instead.
    # Measured over six seeds of the tcnn-initialised case and the +-0.3 case (tools/r06_parity_probe.py, profiles/r06_parity_probe.txt):
    # 1 850 .. 15 751 flipped entries of 22.4 M (<= 7e-4), distance without them 7e-6 .. 2.1e-4 of the travel, with them 5e-5 .. 1.5e-3.
    assert r["param_l2_diff_excl"] <= 1e-3 * r["travel"], \
        f"parameters differ by {r['param_l2_diff_excl'] / r['travel']:.3e} of the distance travelled (sign-flipped entries excluded)"
    # (the flow table's only gradients come through the flow-cycle loss, coefficient 0.005, and the warped dynamic features: rounding-
    # sized on most entries it touches -- measured 5.1e-3 of all entries flipped for the flow model, 8.5e-4 for the feature model)
    assert r["n_sign_flipped"] <= (1e-2 if kind in ("flow", "feature") else 2e-3) * r["n_table_entries"], \
        f"{r['n_sign_flipped']} of {r['n_table_entries']} table entries took a sign-sized step in the other direction"
    # ... and the flipped entries are not free: NO table entry may end further apart than both sides' whole Adam travel.  One step
    # moves an entry by lr_k |m_hat_t| / (sqrt(v_hat_t) + eps) <= lr_k B(t) (eps = 1e-15 only shrinks it; L2 weight decay is part
    # of the gradient that enters both moments, so it changes nothing below).  With m_t = (1 - b1) sum_i b1^(t-i) g_i and
    # v_t = (1 - b2) sum_i b2^(t-i) g_i^2, Cauchy-Schwarz gives |m_t| <= (1 - b1) / sqrt(1 - b2) sqrt(sum_{j<t} (b1^2 / b2)^j) sqrt(v_t),
    # and the bias corrections multiply by sqrt(1 - b2^t) / (1 - b1^t):
    #   B(t) = (1 - b1) / sqrt(1 - b2) * sqrt((1 - r^t) / (1 - r)) * sqrt(1 - b2^t) / (1 - b1^t),  r = b1^2 / b2
    # (B(1) = 1; with b1 = 0.9, b2 = 0.99 it grows towards sqrt(1 / (1 - 0.818)) = 2.35: |m_hat / sqrt(v_hat)| <= 1 holds only at the
    # first step).  So |p_hip - p_ref| <= 2 sum_k lr_k max_t<=K B(t) + both sides' fp32 rounding of p (K 2^-24 |p| each, |p| < 1:
    # below 1e-3 of 2 lr_sum for every case here) -> eps_adam = max_t<=K B(t) - 1 + 1e-3.
    b1, b2 = 0.9, 0.99
    rr = b1 * b1 / b2
    B = max((1 - b1) / math.sqrt(1 - b2) * math.sqrt((1 - rr ** t) / (1 - rr)) * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) for t in range(1, K + 1))
    eps_adam = B - 1 + 1e-3
    print(f"[{kind} K={K}] table max abs diff {r['table_max_abs_diff']:.3e} = {r['table_max_abs_diff'] / (2 * r['lr_sum']):.3f} x 2 lr_sum "
          f"(bound 1 + eps = {1 + eps_adam:.3f}); unfiltered param l2 diff / travel {r['param_l2_diff'] / r['travel']:.3e}")
    assert r["table_max_abs_diff"] <= 2 * r["lr_sum"] * (1 + eps_adam), \
        f"a table entry is {r['table_max_abs_diff']:.3e} apart: more than both sides' whole Adam travel 2 x {r['lr_sum']:.3e} x {1 + eps_adam:.3f}"
    if table_init is not None and kind in ("static", "dynamic"):
        # with +-0.3 tables the few flipped entries do not move the unfiltered distance either (measured 5.5e-5 of the travel for
        # the static case, profiles/r06_parity_probe.txt)
        assert r["param_l2_diff"] <= 1e-3 * r["travel"], \
            f"parameters differ by {r['param_l2_diff'] / r['travel']:.3e} of the distance travelled (every entry counted)"
    # (flow / feature: the unfiltered distance is NOT under 1e-3 of the travel -- measured on MI355X 2.8e-3 (flow) and 1.1e-3 (feature),
    # from the 5e-3 / 8.5e-4 of their table entries that flip -- so these cases rely on the max-abs bound above)
    # ... and no MLP / embedding parameter is further apart than a few of Adam's (sign-sized) steps at the final learning rate
    lr_end = 0.01
    for name, st in r["param_stats"].items():
        if not name.endswith("tcnn_encoding.params"):
            assert st["max_abs_diff"] <= 3 * lr_end, f"{name}: {st['max_abs_diff']:.3e}"


def test_graph_and_eager_training_agree(hip_lib, oracle):
    """The hipGraph-replayed and the eager run of the K-step job end at the same PSNR and the same losses (both were compared with
    the oracle above; this pins them on each other at a tighter bar)."""
    a, b = _run("static", 30, False, 0.3), _run("static", 30, True, 0.3)
    assert max(abs(x - y) / abs(x) for x, y in zip(a["hip_losses"], b["hip_losses"])) <= 2e-4
    assert abs(a["hip_psnr_vs_gt_db"] - b["hip_psnr_vs_gt_db"]) <= 0.02
