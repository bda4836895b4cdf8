"""The video-frame rules without a GPU: the numpy restatement (tests/_frame_ref.py) against the recording of the reference's
``save_concatenated_videos`` / ``save_seperate_videos`` (tests/golden/video_frames.npz; record_video_frames.py), the package's
turbo table, the conditions the fixture's depth probes must meet, and the host-side pieces of ``ops`` / ``video_utils``.

``save_videos`` itself composes on the device also when it is given numpy lists: its recording test is in
tests/test_frames_gpu.py."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

from tests import _frame_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture():
    z = np.load(os.path.join(GOLDEN, "video_frames.npz"))
    z = {k: z[k] for k in z.files}
    return z, json.loads(str(z["meta"]))


def case_results(z, case):
    """render_results of a case as lists of numpy images (with the empty ``dynamic_rgbs`` list the recording ran with)."""
    prefix = case["inputs"] + "/in/"
    res = {k[len(prefix):]: [a for a in v] for k, v in z.items() if k.startswith(prefix)}
    res["dynamic_rgbs"] = []
    return res


def recorded_frames(z, name):
    n = sum(k.startswith(name + "/frame/") for k in z)
    return [z[f"{name}/frame/{i}"] for i in range(n)]


def test_restatement_reproduces_every_recorded_frame():
    """Colour, mask and sky tiles bit for bit; a depth pixel's recorded row is the restatement's own ``t`` choice -- so the whole
    frame equals the first of the three versions.  The order of the frames, the returned frames and the per-view images too."""
    z, meta = load_fixture()
    assert set(meta["cases"]) == {"A_cat", "A_plain", "A_sep", "B_cat", "B_sep"}
    for name, c in meta["cases"].items():
        mine = R.video_frames(case_results(z, c), c["num_timestamps"], c["keys"], c["num_cams"], c["separate"], z["turbo8"])
        rec = recorded_frames(z, name)
        assert len(mine) == len(rec) > 0, name
        for (tag, three), want in zip(mine, rec):
            np.testing.assert_array_equal(three[0], want, err_msg=f"{name} {tag}")
        mid = 0 if c["num_timestamps"] == 1 else c["num_timestamps"] // 2
        by_tag = {tag: three[0] for tag, three in mine}
        returned = {k[len(name) + len("/return/"):]: v for k, v in z.items() if k.startswith(name + "/return/")}
        if c["separate"]:
            assert set(returned) == {tag[0] for tag in by_tag}
            for key, f in returned.items():
                np.testing.assert_array_equal(by_tag[(key, mid)], f)
            # the images of save_images: view j of frame i of a key is its columns of the row
            names = [str(s) for s in z[name + "/image_names"]]
            n = 0
            for tag, three in mine:
                W = three[0].shape[1] // c["num_cams"]
                for j in range(c["num_cams"]):
                    np.testing.assert_array_equal(three[0][:, j * W:(j + 1) * W], z[f"{name}/image/{n}"], err_msg=names[n])
                    n += 1
            assert n == len(names)
        else:
            np.testing.assert_array_equal(by_tag[(mid,)], returned["concatenated_frame"])
    # what the cases are there for
    assert recorded_frames(z, "A_cat")[0].shape == (7 * 6, 3 * 8, 3)       # the absent, the empty and the opacity-less key are skipped
    assert recorded_frames(z, "A_plain")[0].shape == (4 * 6, 3 * 8, 3)
    assert recorded_frames(z, "B_cat")[0].shape == (7 * 5, 7, 3)


def test_fixture_holds_the_probes():
    z, meta = load_fixture()
    f = np.float32
    cols = np.concatenate([z["A/in/gt_rgbs"].ravel(), z["A/in/rgbs"].ravel()])
    for lst in ("A/in/gt_rgbs", "A/in/rgbs"):
        have = set(z[lst].ravel().tolist())
        k = (np.arange(256, dtype=np.float64) / 255).astype(f)
        for probe in (k, np.nextafter(k, f(-1)), np.nextafter(k, f(2))):
            assert set(probe.tolist()) <= have, lst
        for j in range(8):       # two more neighbours on either side of 2^j / 255
            x = f(2.0 ** j / 255)
            for direction in (f(-1), f(2)):
                y = x
                for _ in range(3):
                    y = np.nextafter(y, direction)
                    assert float(y) in have, (lst, j)
    assert (cols < 0).any() and (cols > 1).any() and (cols == 0).any() and (cols == 1).any()
    d, o = z["A/in/static_depths"].ravel(), z["A/in/static_opacities"].ravel()
    for dv in (0.0, -1.0, -1e-6, np.inf, 4.0, 120.0, 3.0, 121.0):
        for ov in (0.0, 1.0, 1 + 1e-7, 1.5):
            assert ((d == f(dv)) & (o == f(ov))).any(), (dv, ov)
        assert ((d == f(dv)) & np.isnan(o)).any(), dv
    assert (np.isnan(d) & (o == 1)).any() and (np.isnan(d) & np.isnan(o)).any()
    mid = R.mid_bin_depths()
    dd, oo = z["A/in/depths"].ravel(), z["A/in/opacities"].ravel()
    at = {float(v): i for i, v in enumerate(dd)}
    idx = np.array([at[float(v)] for v in mid])
    assert (oo[idx] == 1).all()
    rows = R.depth_row_sets(dd[idx], oo[idx])
    np.testing.assert_array_equal(rows[0], np.arange(256))                 # probe k sits in bin k (near depths are the high rows)
    assert all(np.array_equal(r, rows[0]) for r in rows[1:]), "every mid-bin probe has exactly one acceptable row"
    assert meta["numpy"] and meta["matplotlib"]


def test_share_of_ambiguous_depth_pixels_is_small():
    """A condition on the INPUTS, met by the reference's rules alone: at most 1 % of the fixture's depth pixels may have more
    than one acceptable table row (so the GPU test is exact almost everywhere)."""
    z, meta = load_fixture()
    total = ambiguous = 0
    for s in ("A", "B"):
        for dk, ok in (("depths", "opacities"), ("static_depths", "static_opacities"), ("median_depths", "opacities")):
            r0, rm, rp = R.depth_row_sets(z[f"{s}/in/{dk}"], z[f"{s}/in/{ok}"])
            total += r0.size
            ambiguous += int(np.sum((rm != r0) | (rp != r0)))
    assert total >= 3 * (288 + 35)
    assert ambiguous <= 0.01 * total, (ambiguous, total)


def test_turbo_table_is_matplotlibs_and_the_fixtures():
    from emernerf_amd import ops
    z, _ = load_fixture()
    t = ops.turbo_table()
    assert t.shape == (256, 3) and t.dtype == np.float64
    t8 = ops.turbo_table_8bit()
    assert t8.dtype == np.uint8
    np.testing.assert_array_equal(t8, z["turbo8"])                          # recorded from the reference's own colour map
    np.testing.assert_array_equal(t8, np.trunc(255 * t).astype(np.uint8))
    cm = pytest.importorskip("matplotlib").colormaps["turbo"]
    np.testing.assert_array_equal(t, cm(np.arange(256))[:, :3])
    np.testing.assert_array_equal(t, cm(np.linspace(0, 1, 256, endpoint=False) + 1 / 512)[:, :3])


def test_depth_range_and_refusals_on_the_host():
    from emernerf_amd import ops
    dmin, dabs = ops.depth_range()
    assert (dmin, dabs) == tuple(float(v) for v in R.depth_range())
    assert dmin == -np.log(120 + 1e-6) and dabs == abs(-np.log(120 + 1e-6) + np.log(4.0 + 1e-6))
    for kw in (dict(lo=None), dict(hi=None), dict(lo=None, hi=None)):
        with pytest.raises(NotImplementedError, match="percentile"):
            ops.depth_range(**kw)


def test_frame_plan_follows_the_restatement():
    from emernerf_amd import video_utils as V
    z, meta = load_fixture()
    for name, c in meta["cases"].items():
        res = case_results(z, c)
        got = [(k, kind) for k, kind, _, _ in V._frame_plan(res, c["keys"], c["separate"])]
        assert got == [(k, kind) for k, kind, _, _ in R.frame_plan(res, c["keys"], c["separate"])], name
    res = case_results(z, meta["cases"]["A_cat"])
    with pytest.raises(KeyError):          # the separate mode has no fallback for a depth key without its opacity list
        V._frame_plan(res, ["rgbs", "dynamic_depths"], True)
    with pytest.raises(KeyError):
        V._frame_plan(res, ["median_depths"], True)
    assert [p[0] for p in V._frame_plan(res, ["median_depths", "dynamic_depths"], False)] == ["median_depths"]


def test_tile_struct_and_limit_match_the_header():
    from emernerf_amd import ops
    src = open(os.path.join(ROOT, "include", "emernerf_hip.h")).read()
    assert int(re.search(r"#define EMER_FRAME_TILES_MAX (\d+)", src).group(1)) == ops.FRAME_TILES_MAX
    for name, value in ops.TILE_KINDS.items():
        assert int(re.search(rf"#define EMER_TILE_{name.upper()} (\d+)", src).group(1)) == value
    assert ctypes.sizeof(ops._FrameTile) == 32
    assert ops.FRAME_TILES_MAX * ctypes.sizeof(ops._FrameTile) <= 2048      # well under the 4 KiB of kernel arguments


def test_default_writer_needs_imageio(monkeypatch):
    """Without ``writer_factory`` the functions import imageio when they open the writer and say so when it is absent."""
    from emernerf_amd import video_utils as V
    monkeypatch.setitem(sys.modules, "imageio", None)       # import imageio -> ImportError, installed or not
    for fn in (V.save_videos, V.save_concatenated_videos):
        with pytest.raises(ImportError, match="writer_factory"):
            fn({"rgbs": [np.zeros((2, 2, 3), np.float32)]}, "x.mp4", num_timestamps=1, keys=["rgbs"], num_cams=1)
