"""Record the video-frame fixture by running the REFERENCE's own Python on CPU (build container only), on the helpers of
make_golden.py and record_colours.py (which stay as they are):

    python tests/golden/record_video_frames.py

video_frames.npz: radiance_fields/video_utils.py's ``save_concatenated_videos`` and ``save_seperate_videos`` UNMODIFIED on
hand-made ``render_results`` (no model is needed), with utils/visualization_tools.py UNMODIFIED loaded by file location and its
``visualize_depth`` / ``to8b`` / ``resize_five_views`` bound on the video module (which imported stubs of them), matplotlib's
own ``turbo`` map underneath.  ``imageio`` is a stub whose writers collect the frames given to ``append_data`` and whose
``imwrite`` collects names and images.

Inputs (``<set>/in/<key>``: the list stacked to one array):
  * ``A``: 3 cameras x 2 timesteps of 6 x 8 images (24 pixels per frame row: groups of four pixels on dword boundaries);
  * ``B``: 1 camera x 1 timestep of 5 x 7 (byte stores, scalar loads; the returned frame is frame 0).
Keys: gt_rgbs, rgbs, depths, static_depths, median_depths (no ``median_opacities``: falls back to ``opacities``), gt_sky_masks,
sky_masks (read from ``opacities``), and -- merged mode only -- an absent key, an empty list and ``dynamic_depths`` without an
opacity list.  Probe values: colours 0, 1, below 0, above 1, the three fp32 neighbours of every k / 255, and around every
2^j / 255 (where 255 x is nearest to a rounding tie of the fp32 product just below a power of two) two more neighbours on
either side; depths 0, negative, -1e-6, inf, NaN, 4, 120, below 4, above 120, one at the middle of each of the 256 table bins
(opacity 1), log-uniform ones elsewhere; opacities 0, 1, 1 + 1e-7, 1.5, NaN.
Cases (``meta`` holds their arguments as JSON): ``A_cat`` (every key, merged: fp64 scaling), ``A_plain`` (no depth key, merged:
fp32 scaling), ``A_sep`` (separate, save_images), ``B_cat``, ``B_sep``.  Stored per case: every frame in the order written
(``<case>/frame/<n>`` with ``<case>/tags``), the returned frames, the writers' paths and keyword arguments, the image names and
images.  The numpy and matplotlib versions are in ``meta``.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tests import _frame_ref as R  # noqa: E402
from tests.golden import record_colours as RC  # noqa: E402

SEED = 1900
ALL_KEYS = ["gt_rgbs", "rgbs", "depths", "static_depths", "median_depths", "gt_sky_masks", "sky_masks"]
ODD_KEYS = ["shadow_reduced_static_rgbs", "dynamic_rgbs", "dynamic_depths"]        # absent | empty | a depth key without opacities
CASES = {
    "A_cat": dict(inputs="A", keys=ALL_KEYS[:5] + ODD_KEYS + ALL_KEYS[5:], num_cams=3, num_timestamps=2, separate=False, save_pth="out/video.mp4"),
    "A_plain": dict(inputs="A", keys=["gt_rgbs", "rgbs", "gt_sky_masks", "sky_masks"], num_cams=3, num_timestamps=2, separate=False,
                    save_pth="out/plain.mp4"),
    "A_sep": dict(inputs="A", keys=["gt_rgbs", "rgbs", "depths", "static_depths", "gt_sky_masks", "sky_masks", ODD_KEYS[0]], num_cams=3,
                  num_timestamps=2, separate=True, save_pth="out/video.mp4"),
    "B_cat": dict(inputs="B", keys=ALL_KEYS, num_cams=1, num_timestamps=1, separate=False, save_pth="out/image.png"),
    "B_sep": dict(inputs="B", keys=["gt_rgbs", "rgbs", "depths", "static_depths", "gt_sky_masks"], num_cams=1, num_timestamps=1, separate=True,
                  save_pth="out/image.png"),
}


def colour_probes():
    f = np.float32
    k = (np.arange(256, dtype=np.float64) / 255).astype(f)
    vals = [f(0), f(1), f(-0.25), f(-1e-8), f(1.5), f(1 + 1e-6)]
    vals += list(np.nextafter(k, f(-1))) + list(k) + list(np.nextafter(k, f(2)))
    for j in range(8):
        x = f(2.0 ** j / 255)
        lo2, hi2 = np.nextafter(np.nextafter(x, f(-1)), f(-1)), np.nextafter(np.nextafter(x, f(2)), f(2))
        vals += [np.nextafter(lo2, f(-1)), lo2, hi2, np.nextafter(hi2, f(2))]
    return np.array(vals, dtype=f)


DEPTH_SPECIALS = np.array([0.0, -1.0, -1e-6, np.inf, np.nan, 4.0, 120.0, 3.0, 0.5, 121.0, 1e4], dtype=np.float32)
OPACITY_SPECIALS = np.array([0.0, 1.0, 1 + 1e-7, 1.5, np.nan], dtype=np.float32)


def make_inputs(n_images, H, W, seed, with_mid_bins):
    rng = np.random.default_rng(seed)
    n = n_images * H * W
    probes = colour_probes()
    res = {}
    for i, key in enumerate(("gt_rgbs", "rgbs")):
        flat = rng.uniform(-0.1, 1.1, 3 * n).astype(np.float32)
        part = probes if 3 * n >= len(probes) else probes[i::2]        # the small set takes every other probe per list
        m = min(len(part), 3 * n)
        flat[rng.permutation(3 * n)[:m]] = part[:m]
        res[key] = flat.reshape(n_images, H, W, 3)
    grid = np.array([(d, o) for d in DEPTH_SPECIALS for o in OPACITY_SPECIALS], dtype=np.float32)      # 55 pairs
    for j, (dk, ok) in enumerate((("depths", "opacities"), ("static_depths", "static_opacities"), ("median_depths", None),
                                  ("dynamic_depths", None))):
        d = np.exp(rng.uniform(np.log(2.0), np.log(200.0), n)).astype(np.float32)
        o = np.clip(rng.uniform(-0.1, 1.2, n), 0, 1).astype(np.float32)
        where = rng.permutation(n)
        if j == 0:
            if with_mid_bins:
                mid = R.mid_bin_depths()
                d[where[:256]], o[where[:256]] = mid, 1.0
                d[where[256:256 + len(DEPTH_SPECIALS)]] = DEPTH_SPECIALS
            else:
                m = min(n, len(grid))
                d[where[:m]], o[where[:m]] = grid[:m, 0], grid[:m, 1]
        elif j == 1:
            m = min(n, len(grid))
            d[where[:m]], o[where[:m]] = grid[:m, 0], grid[:m, 1]
        res[dk] = d.reshape(n_images, H, W)
        if ok is not None:
            res[ok] = o.reshape(n_images, H, W)
    res["gt_sky_masks"] = (rng.uniform(0, 1, n) < 0.4).astype(np.float32).reshape(n_images, H, W)
    return res


def as_lists(stacked):
    """render_results as the loop returns it: lists of per-image arrays; ``dynamic_rgbs`` is there and empty."""
    res = {k: [a.copy() for a in v] for k, v in stacked.items()}
    res["dynamic_rgbs"] = []
    return res


class Recorder:
    """What the imageio stub collects."""

    def __init__(self):
        self.writers, self.frames, self.images = [], [], []

    def get_writer(self, path, **kw):
        rec = self
        rec.writers.append((path, kw))

        class W:
            def append_data(self, frame):
                rec.frames.append((path, np.array(frame)))

            def close(self):
                pass
        return W()

    def imwrite(self, path, image):
        self.images.append((path, np.array(image)))


def main():
    import matplotlib
    vt = RC._load_visualization_tools()
    from radiance_fields import video_utils as ref_video
    ref_video.visualize_depth, ref_video.to8b, ref_video.resize_five_views = vt.visualize_depth, vt.to8b, vt.resize_five_views
    ref_video.trange = lambda n, **k: range(n)
    table = vt.turbo_cmap(np.arange(256))[:, :3]
    out = {"turbo8": (255 * np.clip(table, 0, 1)).astype(np.uint8)}
    inputs = {"A": make_inputs(6, 6, 8, SEED, True), "B": make_inputs(1, 5, 7, SEED + 1, False)}
    for name, stacked in inputs.items():
        for k, v in stacked.items():
            out[f"{name}/in/{k}"] = v
    import tempfile
    cwd, tmp = os.getcwd(), tempfile.TemporaryDirectory()
    os.chdir(tmp.name)      # save_images makes directories next to save_pth
    try:
        for case, c in CASES.items():
            rec = Recorder()
            ref_video.imageio.get_writer, ref_video.imageio.imwrite = rec.get_writer, rec.imwrite
            fn = ref_video.save_seperate_videos if c["separate"] else ref_video.save_concatenated_videos
            kw = dict(save_images=True) if c["separate"] else {}
            ret = fn(as_lists(inputs[c["inputs"]]), c["save_pth"], num_timestamps=c["num_timestamps"], keys=list(c["keys"]), num_cams=c["num_cams"],
                     verbose=False, **kw)
            assert all(f.dtype == np.uint8 for _, f in rec.frames)
            out[f"{case}/tags"] = np.array([p for p, _ in rec.frames])
            for n, (_, f) in enumerate(rec.frames):
                out[f"{case}/frame/{n}"] = f
            for k, f in ret.items():
                out[f"{case}/return/{k}"] = f
            out[f"{case}/writers"] = np.array([json.dumps([p, kw_]) for p, kw_ in rec.writers])
            out[f"{case}/image_names"] = np.array([p for p, _ in rec.images] or [""])
            for n, (_, im) in enumerate(rec.images):
                out[f"{case}/image/{n}"] = im
    finally:
        os.chdir(cwd)
        tmp.cleanup()
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "matplotlib": matplotlib.__version__, "cases": CASES, "lo": R.LO, "hi": R.HI}))
    path = os.path.join(HERE, "video_frames.npz")
    np.savez_compressed(path, **out)
    print(f"video_frames: {len(out)} arrays, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
