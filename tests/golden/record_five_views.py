"""Record the five-view fixture by running the REFERENCE's own Python on CPU (build container only; needs scipy and matplotlib),
on the helpers of record_video_frames.py and record_colours.py (which stay as they are):

    python tests/golden/record_five_views.py

five_views.npz: radiance_fields/video_utils.py's ``save_concatenated_videos`` and ``save_seperate_videos`` UNMODIFIED on hand-made
``render_results`` of FIVE cameras, with utils/visualization_tools.py UNMODIFIED -- its REAL ``resize_five_views``
(``scipy.ndimage.zoom``), ``visualize_depth`` and ``to8b`` -- bound on the video module, matplotlib's own ``turbo`` map
underneath, and ``imageio`` a stub that collects what it is given.

Cases (``meta`` holds their arguments as JSON):
  * ``M``: merged, 2 timesteps, 16 x 32 images (h = 14), keys gt_rgbs, rgbs, depths, gt_sky_masks, sky_masks: fp64 scaling;
  * ``S``: separate, 1 timestep, 37 x 53 (h = 24, odd sizes), keys rgbs, depths, save_images;
  * ``E``: merged, 1 timestep, 9 x 20 (h = 9 = H: no black rows), keys rgbs, depths.
Inputs.  The fixture stays small by storing what cannot be regenerated bit for bit and a seed for the rest: ``make_inputs`` below
IS the input generator, for the recording and for the tests.  Colours are seeded uniform fp32 values in [-0.1, 1.1] with a few
0 and 1 probes and, in ``rgbs``, six constant columns of 1 (whose zoom is 1 -+ 1e-16 in fp64: 254 or 255 without the rounding
to fp32), ``gt_sky_masks`` seeded 0 / 1; both come from numpy's Generator alone (no libm) and a checksum of every list is
stored (``<case>/sum/<key>``).  Depths of the RESIZED views (0 and 4) are mid-bin depths (``_frame_ref.mid_bin_depths``: stored as
``mid_bin_depths`` with one stored bin index per pixel) under opacities from {0, 0.25, 0.5, 1} (a stored index): such a pixel has
ONE acceptable table row, so the zoom's input is exact.  The middle views have seeded uniform depths in [2, 200] and
opacities in [0, 1], whose table rows may be ambiguous as in every frame test.
Stored per case: every frame in the order written (``<case>/frame/<n>``, ``<case>/tags``), the returned frames (as the number of
the written frame each one is), the writers, the
image names (each image is checked here to be its view's columns of the frame, and not stored).  And scipy's own outputs for the
outer views of timestep 0, as the reference calls it (``ndimage.zoom(img, [h / H, 1, 1])``): ``<case>/zoom32/<key>/<view>`` for the
fp32 lists (the mask keys: one of their three equal channels), ``<case>/zoom64/depths/<view>`` for the fp64 depth colours (``S``: view 0 only), and
``<case>/zoom64/rgbs/0``: the zoom of view 0's colours cast to fp64.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _frame_ref as R  # noqa: E402

OPACITY_LEVELS = np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32)
CASES = {
    "M": dict(H=16, W=32, seed=2501, keys=["gt_rgbs", "rgbs", "depths", "gt_sky_masks", "sky_masks"], num_cams=5, num_timestamps=2,
              separate=False, save_pth="out/video.mp4"),
    "S": dict(H=37, W=53, seed=2502, keys=["rgbs", "depths"], num_cams=5, num_timestamps=1, separate=True, save_pth="out/image.png"),
    "E": dict(H=9, W=20, seed=2503, keys=["rgbs", "depths"], num_cams=5, num_timestamps=1, separate=False, save_pth="out/edge.png"),
}


def make_inputs(c, mid, bins=None, levels=None):
    """(render_results as lists of per-image arrays, bin indices, opacity-level indices) of a case.  ``mid``: the 256 mid-bin
    depths; ``bins`` / ``levels`` [n_images, H, W] uint8: the recorded indices (drawn here when None: the recording)."""
    H, W, n = c["H"], c["W"], c["num_cams"] * c["num_timestamps"]
    rng = np.random.default_rng(c["seed"])
    res = {}
    for key in ("gt_rgbs", "rgbs"):
        a = rng.uniform(-0.1, 1.1, (n, H, W, 3)).astype(np.float32)
        flat = a.reshape(n, -1)
        flat[:, :4] = [0.0, 1.0, 1.0, 0.0]
        if key == "rgbs":       # constant columns: the zoom gives 1 -+ 1e-16 in fp64, which only the rounding to fp32 makes 255 again
            a[:, :, 8:14] = 1.0
        res[key] = a
    res["gt_sky_masks"] = (rng.uniform(0, 1, (n, H, W)) < 0.5).astype(np.float32)
    depth = rng.uniform(2.0, 200.0, (n, H, W)).astype(np.float32)
    opacity = rng.uniform(0.0, 1.0, (n, H, W)).astype(np.float32)
    if bins is None:
        bins = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
        levels = rng.integers(0, 4, (n, H, W)).astype(np.uint8)
    for i in range(n):
        if i % c["num_cams"] in (0, 4):
            depth[i], opacity[i] = np.asarray(mid, dtype=np.float32)[bins[i]], OPACITY_LEVELS[levels[i]]
    res["depths"], res["opacities"] = depth, opacity
    return {k: [a for a in v] for k, v in res.items()}, bins, levels


def checksum(images):
    return float(np.sum(np.stack(images).astype(np.float64)))


def main():
    import matplotlib
    import scipy
    from scipy import ndimage
    from tests.golden import record_colours as RC
    from tests.golden.record_video_frames import Recorder
    vt = RC._load_visualization_tools()
    from radiance_fields import video_utils as ref_video
    ref_video.visualize_depth, ref_video.to8b, ref_video.resize_five_views = vt.visualize_depth, vt.to8b, vt.resize_five_views
    ref_video.trange = lambda n, **k: range(n)
    assert vt.resize_five_views.__module__ == vt.__name__ and vt.ndimage is ndimage
    table = vt.turbo_cmap(np.arange(256))[:, :3]
    mid = R.mid_bin_depths()
    out = {"turbo8": (255 * np.clip(table, 0, 1)).astype(np.uint8), "turbo64": table.astype(np.float64), "mid_bin_depths": mid}
    import tempfile
    cwd, tmp = os.getcwd(), tempfile.TemporaryDirectory()
    os.chdir(tmp.name)      # save_images makes directories next to save_pth
    try:
        for case, c in CASES.items():
            res, bins, levels = make_inputs(c, mid)
            out[f"{case}/bins"], out[f"{case}/levels"] = bins, levels
            for k, v in res.items():
                out[f"{case}/sum/{k}"] = np.array(checksum(v))
            rec = Recorder()
            ref_video.imageio.get_writer, ref_video.imageio.imwrite = rec.get_writer, rec.imwrite
            fn = ref_video.save_seperate_videos if c["separate"] else ref_video.save_concatenated_videos
            kw = dict(save_images=True) if c["separate"] else {}
            ret = fn({k: [a.copy() for a in v] for k, v in res.items()}, c["save_pth"], num_timestamps=c["num_timestamps"], keys=list(c["keys"]),
                     num_cams=c["num_cams"], verbose=False, **kw)
            assert all(f.dtype == np.uint8 for _, f in rec.frames)
            out[f"{case}/tags"] = np.array([p for p, _ in rec.frames])
            for n, (_, f) in enumerate(rec.frames):
                out[f"{case}/frame/{n}"] = f
            for k, f in ret.items():        # a returned frame is one of the written ones: its number is stored
                hits = [n for n, (_, g) in enumerate(rec.frames) if g is f or (g.shape == f.shape and np.array_equal(g, f))]
                out[f"{case}/return/{k}"] = np.array(hits[0])
            out[f"{case}/writers"] = np.array([json.dumps([p, kw_]) for p, kw_ in rec.writers])
            out[f"{case}/image_names"] = np.array([p for p, _ in rec.images] or [""])
            W = c["W"]
            for n, (_, im) in enumerate(rec.images):        # every image is its view's columns of the frame
                frame = rec.frames[n // c["num_cams"]][1]
                j = n % c["num_cams"]
                assert np.array_equal(im, frame[:, j * W:(j + 1) * W]), (case, n)
            # scipy's own outputs for the outer views of timestep 0, called as resize_five_views calls it
            h, H = int(W * 0.46), c["H"]
            for view in (0, 4):
                for key in c["keys"]:
                    if key == "depths":
                        img = ref_video.depth_visualizer(res["depths"][view], res["opacities"][view])
                        assert img.dtype == np.float64
                        if case != "S" or view == 0:        # the fixture's size: the largest case keeps one of its two
                            out[f"{case}/zoom64/depths/{view}"] = ndimage.zoom(img, [h / H, W / W, 1])
                        continue
                    if key == "sky_masks":
                        img = 1 - np.stack([res["opacities"][view]] * 3, axis=-1)
                    elif key == "gt_sky_masks":
                        img = np.stack([res[key][view]] * 3, axis=-1)
                    else:
                        img = res[key][view]
                    assert img.dtype == np.float32
                    z = ndimage.zoom(img, [h / H, W / W, 1])
                    assert z.dtype == np.float32 and z.shape == (h, W, 3)
                    out[f"{case}/zoom32/{key}/{view}"] = z[..., 0] if "sky" in key else z
                    if key == "rgbs" and view == 0:
                        out[f"{case}/zoom64/rgbs/0"] = ndimage.zoom(img.astype(np.float64), [h / H, W / W, 1])
    finally:
        os.chdir(cwd)
        tmp.cleanup()
    cases = {k: dict(v) for k, v in CASES.items()}
    out["meta"] = np.array(json.dumps({"numpy": np.__version__, "matplotlib": matplotlib.__version__, "scipy": scipy.__version__, "cases": cases,
                                       "lo": R.LO, "hi": R.HI}))
    path = os.path.join(HERE, "five_views.npz")
    np.savez_compressed(path, **out)
    print(f"five_views: {len(out)} arrays, {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
