"""Record the s -> t fixture by running the REFERENCE's own ``_transform_stot`` (third_party/nerfacc_prop_net.py:299-339, UNMODIFIED)
on the CPU (build container only), imported through the shims of make_golden.py (which stays as it is):

    python tests/golden/record_stot.py

stot_reference.npz holds only numbers: ``s`` (320 fp32 values in [0, 1], among them 0, 0.5, its two neighbours and 1),
``planes`` [3, 2] (t_min, t_max as the floats the reference receives) and, for each of the six transform types and each plane
pair, the reference's result ``t/<type>/<pair>`` as raw fp32.  tests/test_sample_bounds_cpu.py holds the fp32 model of
tests/_sample_probe.py to it: bit for bit for five types, within 1 ulp for ``log`` (the recorder prints the measured distance).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tests.golden import make_golden as G  # noqa: E402

SEED = 1800
N = 320
PLANES = ((0.1, 1000.0), (0.5, 300.0), (1.0, 200.0))      # the shipped planes; another pair; both forward breaks (1 and 200)
TYPES = ("uniform", "lindisp", "sqrt", "log", "uniform_lindisp", "uniform_lindisp_0")


def s_values(seed=SEED, n=N) -> np.ndarray:
    s = np.random.default_rng(seed).random(n).astype(np.float32)
    half = np.float32(0.5)
    s[:6] = [0.0, 0.5, 1.0, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), 0.25]
    return s


def run_case():
    G._install_video_utils_shims()          # nerfacc / tcnn / omegaconf shims, the reference on sys.path
    from third_party import nerfacc_prop_net as ref_prop
    s = s_values()
    out = {"s": s, "planes": np.array(PLANES, np.float64)}
    for typ in TYPES:
        for i, (t_min, t_max) in enumerate(PLANES):
            t = ref_prop._transform_stot(typ, torch.from_numpy(s.copy()), float(t_min), float(t_max))
            assert t.dtype == torch.float32 and t.shape == (N,)
            out[f"t/{typ}/{i}"] = t.numpy().copy()
    return out


def main():
    out = run_case()
    path = os.path.join(HERE, "stot_reference.npz")
    np.savez_compressed(path, **out)
    print(f"stot_reference: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")
    from tests import _sample_probe as P
    for typ in TYPES:
        worst = 0
        for i, planes in enumerate(PLANES):
            want = P.model_stot(typ, out["s"], *planes)
            worst = max(worst, int(np.abs(out[f"t/{typ}/{i}"].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()))
        print(f"  {typ}: largest distance from the fp32 model {worst} ulp")


if __name__ == "__main__":
    main()
