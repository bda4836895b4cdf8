"""The five-view resize without a GPU: the numpy restatement (tests/_zoom_ref.py) against the recording of the reference's
``save_concatenated_videos`` / ``save_seperate_videos`` with its real ``resize_five_views`` (tests/golden/five_views.npz;
record_five_views.py), against scipy's own recorded outputs, and -- where scipy is installed -- against ``ndimage.zoom``
itself; the conditions the fixture must meet; three mutants of the rules that the recording must kill.

The device path is in tests/test_five_views_gpu.py."""
import json
import os

import numpy as np
import pytest

from tests import _frame_ref as R
from tests import _zoom_ref as Z
from tests.golden import record_five_views as REC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def load_fixture():
    if "z" not in _CACHE:
        z = np.load(os.path.join(GOLDEN, "five_views.npz"))
        _CACHE["z"] = {k: z[k] for k in z.files}
    z = _CACHE["z"]
    return z, json.loads(str(z["meta"]))


def case_results(z, name, c):
    """render_results of a case, regenerated from its seed and the stored indices; the stored checksums hold."""
    res, _, _ = REC.make_inputs(c, z["mid_bin_depths"], z[name + "/bins"], z[name + "/levels"])
    for k, v in res.items():
        assert REC.checksum(v) == float(z[f"{name}/sum/{k}"]), f"{name}: the regenerated {k} are not the recorded ones"
    return res


def recorded_frames(z, name):
    n = sum(k.startswith(name + "/frame/") for k in z)
    return [z[f"{name}/frame/{i}"] for i in range(n)]


def restated(name):
    """(case, results, [(tag, three frames)]) -- computed once per case."""
    if name not in _CACHE:
        z, meta = load_fixture()
        c = meta["cases"][name]
        res = case_results(z, name, c)
        _CACHE[name] = (c, res, Z.video_frames(res, c["num_timestamps"], c["keys"], c["num_cams"], c["separate"], z["turbo8"], z["turbo64"]))
    return _CACHE[name]


def outer_tiles(name):
    """(key, kind, image index, src, opacity) of every resized tile of a case."""
    c, res, _ = restated(name)
    out = []
    for key, kind, images, opacities in R.frame_plan(res, c["keys"], c["separate"]):
        for i in range(c["num_timestamps"] * c["num_cams"]):
            if i % c["num_cams"] in (0, 4):
                out.append((key, kind, i, np.asarray(images[i]), None if opacities is None else np.asarray(opacities[i])))
    return out


CASE_NAMES = ["M", "S", "E"]


def test_fixture_is_the_three_cases():
    z, meta = load_fixture()
    assert list(meta["cases"]) == CASE_NAMES
    sizes = {n: (c["H"], c["W"], Z.out_rows(c["W"])) for n, c in meta["cases"].items()}
    assert sizes == {"M": (16, 32, 14), "S": (37, 53, 24), "E": (9, 20, 9)}
    assert not meta["cases"]["M"]["separate"] and meta["cases"]["M"]["num_timestamps"] == 2 and meta["cases"]["S"]["separate"]
    assert all(c["num_cams"] == 5 for c in meta["cases"].values())
    assert os.path.getsize(os.path.join(GOLDEN, "five_views.npz")) < 300_000
    from emernerf_amd import ops
    np.testing.assert_array_equal(ops.turbo_table(), z["turbo64"])
    np.testing.assert_array_equal(ops.turbo_table_8bit(), z["turbo8"])
    assert [ops.five_view_rows(W) for W in (12, 32, 53, 20, 96, 1012)] == [5, 14, 24, 9, 44, 465]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_restatement_reproduces_the_recording(name):
    """Every recorded frame through ``_frame_ref.compare``: each pixel is one of its acceptable values and no more pixels take a
    second choice than have one; the frames come in the recorded order and the returned frames are the recorded ones."""
    z, _ = load_fixture()
    c, _, mine = restated(name)
    rec = recorded_frames(z, name)
    assert len(mine) == len(rec) > 0
    tags = [str(t) for t in z[name + "/tags"]]
    for (tag, three), want, path in zip(mine, rec, tags):
        ok, second, ambiguous = R.compare(want, three)
        print(f"{name} {tag}: {second} recorded pixels off the first choice, {ambiguous} pixels with a choice")
        assert ok, f"{name} {tag}: a recorded pixel is none of the restatement's"
        assert second <= ambiguous
        if c["separate"]:
            assert path == c["save_pth"].replace(".png", f"_{tag[0]}.png").replace(".mp4", f"_{tag[0]}.mp4")
    mid = 0 if c["num_timestamps"] == 1 else c["num_timestamps"] // 2
    returned = {k[len(name) + len("/return/"):]: int(v) for k, v in z.items() if k.startswith(name + "/return/")}
    want = {key: n for n, (tag, _) in enumerate(mine) if tag[-1] == mid for key in ([tag[0]] if c["separate"] else ["concatenated_frame"])}
    assert returned == want
    if c["separate"]:
        names = [str(s) for s in z[name + "/image_names"]]
        paths = {key: c["save_pth"].replace(".mp4", f"_{key}.mp4").replace(".png", f"_{key}.png") for key, _ in [tag for tag, _ in mine]}
        assert names == [paths[key].replace(".mp4", f"_{i * 3 + j:03d}.png") for (key, i), _ in mine for j in range(5)]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_recorded_scipy_values_lie_within_the_bound(name):
    """scipy's own zoom outputs of the outer views: every fp64 value within ``e`` of ``v``, every fp32 value between the fp32
    roundings of ``v - e`` and ``v + e``; and ``e <= 2^-40`` everywhere."""
    z, _ = load_fixture()
    c, res, _ = restated(name)
    h = Z.out_rows(c["W"])
    seen = 0
    worst = 0.0
    for key, kind, i, src, opacity in outer_tiles(name):
        v, e = Z.zoom_values(kind, src, opacity, h, z["turbo64"])
        assert v.shape == (h, c["W"], 3) and float(e.max()) <= 2.0 ** -40, (key, float(e.max()))
        k64, k32 = f"{name}/zoom64/{key}/{i}", f"{name}/zoom32/{key}/{i}"
        if k64 in z:
            d = np.abs(z[k64] - v)
            worst = max(worst, float(np.max(d / np.maximum(e, 1e-300))))
            assert np.all(d <= e), f"{k64}: {float(np.max(d - e))} over the bound"
            seen += 1
        if k32 in z:
            s = z[k32] if z[k32].ndim == 3 else np.repeat(z[k32][..., None], 3, axis=-1)
            assert s.dtype == np.float32
            assert np.all(((v - e).astype(np.float32) <= s) & (s <= (v + e).astype(np.float32))), k32
            seen += 1
    print(f"{name}: {seen} recorded arrays, the largest |scipy - v| / e = {worst:.3g}")
    assert seen == {"M": 11, "S": 4, "E": 5}[name]


def choice_share(name, **mutant):
    """(resized pixels with more than one acceptable byte triple -- v - e and v + e on two sides of a byte's edge --, resized pixels)."""
    z, _ = load_fixture()
    c, res, _ = restated(name)
    n_px = n_choice = 0
    merged_fp64 = (not c["separate"]) and "depths" in c["keys"]
    for key, kind, i, src, opacity in outer_tiles(name):
        t0, tm, tp = Z.resized_tile8(kind, src, opacity, merged_fp64, z["turbo64"], **mutant)
        n_px += t0.shape[0] * t0.shape[1]
        n_choice += int(np.sum(np.any(tm != t0, axis=-1) | np.any(tp != t0, axis=-1)))
    return n_choice, n_px


@pytest.mark.parametrize("name", CASE_NAMES)
def test_resized_depth_pixels_have_one_table_row_and_few_pixels_a_choice(name):
    """The zoom's input must be exact: every depth pixel of a resized view has ONE acceptable table row.  And at most 1 in 1000
    resized pixels has more than one acceptable byte triple: a test that accepts either byte there checks nothing."""
    for key, kind, i, src, opacity in outer_tiles(name):
        if kind == "depth":
            r0, rm, rp = R.depth_row_sets(src, opacity)
            assert np.array_equal(r0, rm) and np.array_equal(r0, rp), f"{name} {key} image {i}: a depth pixel with two acceptable rows"
    n_choice, n_px = choice_share(name)
    print(f"{name}: {n_choice} of {n_px} resized pixels have a choice")
    assert n_choice * 1000 <= n_px


@pytest.mark.parametrize("mutant", [dict(mirror=False), dict(rule="grid"), dict(round32=False)], ids=["ends", "coordinate", "round32"])
def test_the_recording_kills_the_mutants(mutant):
    """Ends that see zeros instead of the mirror image, the H / h coordinate rule, and no rounding to fp32 before the clip: the
    checks above refuse each on the merged case -- a recorded pixel that is none of the mutant's, or (the missing rounding: a
    constant column of 1 zooms to 1 -+ 1e-16, which is 254 or 255) more than 1 in 1000 resized pixels left with a choice."""
    z, _ = load_fixture()
    c, res, _ = restated("M")
    frames = Z.video_frames(res, c["num_timestamps"], c["keys"], c["num_cams"], c["separate"], z["turbo8"], z["turbo64"], **mutant)
    refused = 0
    for (tag, three), want in zip(frames, recorded_frames(z, "M")):
        ok, second, ambiguous = R.compare(want, three)
        refused += (not ok) or second > ambiguous
    n_choice, n_px = choice_share("M", **mutant)
    print(f"{mutant}: {refused} frames refused, {n_choice} of {n_px} resized pixels with a choice")
    assert refused > 0 or n_choice * 1000 > n_px
    if "round32" not in mutant:
        assert refused > 0


@pytest.mark.parametrize("H,W", [(200, 96), (300, 300), (520, 1012)])
def test_restatement_agrees_with_scipy(H, W):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(H + W)
    h = Z.out_rows(W)
    a = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)
    v, e = Z.zoom_columns(a, h)
    s64 = ndimage.zoom(a.astype(np.float64), [h / H, 1, 1])
    assert s64.shape == v.shape
    print(f"{H} x {W}: max |scipy - v| = {float(np.abs(s64 - v).max()):.3g}, max e = {float(e.max()):.3g}")
    assert np.all(np.abs(s64 - v) <= e) and float(e.max()) <= 2.0 ** -40
    s32 = ndimage.zoom(a, [h / H, 1, 1])
    assert s32.dtype == np.float32 and np.all(((v - e).astype(np.float32) <= s32) & (s32 <= (v + e).astype(np.float32)))


def test_refusals_of_the_restatement():
    a = np.zeros((8, 40, 3), np.float32)
    with pytest.raises(ValueError):
        Z.zoom_columns(a, Z.out_rows(40))         # h = 18 > H = 8
    with pytest.raises(ValueError):
        Z.zoom_columns(np.zeros((8, 4, 3), np.float32), Z.out_rows(4))       # h = 1
