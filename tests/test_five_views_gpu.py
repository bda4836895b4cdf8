"""The five-view resize on the GPU (csrc/frames.hip ``zoom_tiles_kernel``; ``ops.zoom_rows`` / ``ops.five_view_frame``;
``video_utils`` with ``five_view_resize="zoom"``): the values against the numpy restatement of tests/_zoom_ref.py within its
per-entry bound ``e``, the frames against the recording of the reference's own ``save_concatenated_videos`` /
``save_seperate_videos`` with its real ``resize_five_views`` (tests/golden/five_views.npz)."""
import json

import numpy as np
import pytest
import torch

from tests import _frame_ref as R
from tests import _zoom_ref as Z
from tests.test_five_views_cpu import load_fixture, recorded_frames, restated
from tests.test_frames_gpu import Writers, assert_frame, dev, plan_tiles, to_device

pytestmark = pytest.mark.gpu

BLOCK_ROWS, WARM = 32, 36        # csrc/frames.hip: kZoomRows, kZoomWarm
SHAPES = [(8, 12), (37, 53), (16, 32), (9, 20), (200, 96), (520, 1012)]


def exact_depths(H, W, rng):
    """A depth image whose every pixel has ONE acceptable table row: mid-bin depths under opacities from {0, 0.25, 0.5, 1}."""
    depth = R.mid_bin_depths()[rng.integers(0, 256, (H, W))]
    opacity = np.array([0.0, 0.25, 0.5, 1.0], np.float32)[rng.integers(0, 4, (H, W))]
    r0, rm, rp = R.depth_row_sets(depth, opacity)
    assert np.array_equal(r0, rm) and np.array_equal(r0, rp)
    return depth, opacity


def inputs(H, W):
    """[(what, kind, src, opacity)]: uniform values on every kind, and on colour tiles the constants, the pole's worst case and
    one bright row per column and channel, placed at every distance up to WARM from the first block seam."""
    rng = np.random.default_rng(1000 * H + W)
    out = [("uniform", "colour3", rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32), None),
           ("uniform", "grey1", rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32), None),
           ("uniform", "one_minus_grey1", rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32), None),
           ("mid-bin", "depth", *exact_depths(H, W, rng)),
           ("zeros", "colour3", np.zeros((H, W, 3), np.float32), None),
           ("ones", "colour3", np.ones((H, W, 3), np.float32), None)]
    alt = np.zeros((H, W, 3), np.float32)
    alt[1::2] = 1.0
    out.append(("alternating rows", "colour3", alt, None))
    bright = np.zeros((H, 3 * W), np.float32)
    j = np.arange(3 * W)
    bright[(BLOCK_ROWS - WARM + j) % H, j] = 1.0
    out.append(("one bright row", "colour3", bright.reshape(H, W, 3), None))
    return out


@pytest.mark.parametrize("H,W", SHAPES)
def test_zoom_rows_within_the_bound_on_every_path(hip_lib, H, W):
    """8 x 12: one block, the warm-up longer than the image; 37 x 53 and 9 x 20 (h = H): odd sizes; 200 x 96 and 520 x 1012:
    many row blocks and their seams, several lane groups.  Every entry within ``e`` of the restatement."""
    from emernerf_amd import ops
    z, _ = load_fixture()
    h = Z.out_rows(W)
    if (H, W) in ((200, 96), (520, 1012)):
        assert H > 2 * BLOCK_ROWS + WARM
    for what, kind, src, opacity in inputs(H, W):
        v, e = Z.zoom_values(kind, src, opacity, h, z["turbo64"])
        got = ops.zoom_rows(dev(src), h, kind, None if opacity is None else dev(opacity))
        assert got.dtype == torch.float64 and tuple(got.shape) == (h, W, 3)
        d = np.abs(got.cpu().numpy() - v)
        with np.errstate(all="ignore"):
            print(f"{H} x {W} {what} {kind}: max |got - v| = {float(d.max()):.3g}, max e = {float(e.max()):.3g}, "
                  f"max ratio = {float(np.nanmax(np.where(e > 0, d / e, 0))):.3g}")
        assert np.all(d <= e), f"{H} x {W} {what} {kind}: {int(np.sum(d > e))} entries over the bound, by up to {float(np.max(d - e)):.3g}"


def five_tiles(H, W, seed, offset=0):
    """One colour row of five seeded views as (numpy tiles, device tiles)."""
    rng = np.random.default_rng(seed)
    tiles = [("colour3", 0, c, rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32), None) for c in range(5)]
    return tiles, to_device(tiles, offset)


def test_views_into_their_storage_give_the_same_bytes(hip_lib):
    """16 x 32 (rows of whole 16-byte quads) from aligned tensors and from views 1 and 3 floats into their storage."""
    from emernerf_amd import ops
    z, _ = load_fixture()
    H, W = 16, 32
    tiles, on_dev = five_tiles(H, W, 5)
    for flag in (False, True):
        got = ops.five_view_frame(on_dev, H, W, 1, flag)
        assert_frame(got.cpu().numpy(), Z.compose(tiles, H, W, 1, 5, flag, z["turbo8"], z["turbo64"]), f"16 x 32 fp64={flag}")
        for offset in (1, 3):
            view = ops.five_view_frame(to_device(tiles, offset), H, W, 1, flag)
            assert torch.equal(view, got), f"a view {offset} floats into its storage gives other bytes"


# ------------------------------------------------------------------------------------------------- against the recording
@pytest.mark.parametrize("name", ["M", "E"])
def test_five_view_frame_matches_recording(hip_lib, name):
    """The merged frames of the recording from ``ops.five_view_frame``; the columns of views 1 to 3 are bit-equal to
    ``compose_frame`` alone."""
    from emernerf_amd import ops
    z, _ = load_fixture()
    c, res, mine = restated(name)
    plan = R.frame_plan(res, c["keys"], False)
    fp64 = any(kind == "depth" for _, kind, _, _ in plan)
    rec = recorded_frames(z, name)
    H, W = c["H"], c["W"]
    for i in range(c["num_timestamps"]):
        tiles = plan_tiles(plan, i, 5)
        got = ops.five_view_frame(tiles, H, W, len(plan), fp64)
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (len(plan) * H, 5 * W, 3)
        three = mine[i][1]
        assert_frame(got.cpu().numpy(), three, f"{name} frame {i}")
        assert_frame(got.cpu().numpy(), (rec[i], three[1], three[2]), f"{name} frame {i} vs the recording")
        middle = ops.compose_frame([t for t in tiles if t[2] in (1, 2, 3)], H, W, len(plan), 5, fp64)
        assert torch.equal(got[:, W:4 * W], middle[:, W:4 * W])
        assert int(middle[:, :W].sum()) == 0 and int(middle[:, 4 * W:].sum()) == 0


@pytest.mark.parametrize("source", ["numpy", "device"])
@pytest.mark.parametrize("name", ["M", "S", "E"])
def test_save_videos_matches_recording(hip_lib, name, source, tmp_path, monkeypatch):
    """``save_videos(..., five_view_resize="zoom")`` with a recording writer hands over the recorded frames in the recorded order,
    opens the recorded writers, writes the recorded image names and returns the recorded frame; ``compose_video_frames`` yields
    the same frames.  From numpy lists and from device tensors."""
    from emernerf_amd import video_utils as V
    z, _ = load_fixture()
    c, res, mine = restated(name)
    if source == "device":
        res = {k: [dev(a) for a in v] for k, v in res.items()}
    rec = recorded_frames(z, name)
    tags = [str(t) for t in z[name + "/tags"]]
    monkeypatch.chdir(tmp_path)          # save_images makes its directories next to save_pth
    w = Writers()
    ret = V.save_videos(res, c["save_pth"], c["num_timestamps"], keys=list(c["keys"]), num_cams=5, save_seperate_video=c["separate"],
                        save_images=c["separate"], verbose=False, writer_factory=w.factory, image_writer=w.imwrite, five_view_resize="zoom")
    assert [p for p, _ in w.frames] == tags
    for (path, f), want, (tag, three) in zip(w.frames, rec, mine):
        assert isinstance(f, np.ndarray) and f.dtype == np.uint8
        assert_frame(f, (want, three[1], three[2]), f"{name} {tag} ({source})")
    recorded_writers = [tuple(json.loads(str(s))) for s in z[name + "/writers"]]
    used = [(p, kw) for p, kw in recorded_writers if p in tags]
    assert [(p, kw) for p, kw in w.opened] == used and w.closed == [p for p, _ in used]
    returned = {k[len(name) + len("/return/"):]: int(v) for k, v in z.items() if k.startswith(name + "/return/")}
    assert set(ret) == set(returned)
    for k, f in ret.items():
        three = mine[returned[k]][1]
        assert_frame(f, (rec[returned[k]], three[1], three[2]), f"{name}: returned {k}")
    if c["separate"]:
        names = [str(s) for s in z[name + "/image_names"]]
        assert [p for p, _ in w.images] == names
        W = c["W"]
        for n, (_, im) in enumerate(w.images):      # the recorded image is its view's columns of the recorded frame
            want, three = rec[n // 5], mine[n // 5][1]
            j = n % 5
            assert_frame(im, tuple(t[:, j * W:(j + 1) * W] for t in (want, three[1], three[2])), names[n])
    frames = list(V.compose_video_frames(res, c["num_timestamps"], list(c["keys"]), 5, separate=c["separate"], five_view_resize="zoom"))
    assert [f[:-1] for f in frames] == [tag for tag, _ in mine]
    for f, (path, g) in zip(frames, w.frames):
        np.testing.assert_array_equal(f[-1], g)


# ------------------------------------------------------------------------------------------------------------ independence
def test_a_resized_tiles_bytes_do_not_depend_on_its_row_or_its_neighbours(hip_lib):
    from emernerf_amd import ops
    H, W = 16, 32
    rng = np.random.default_rng(11)
    kinds = [("colour3", rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32), None),
             ("grey1", rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32), None),
             ("one_minus_grey1", rng.uniform(-0.2, 1.2, (H, W)).astype(np.float32), None),
             ("depth", *exact_depths(H, W, rng))]
    _, other = five_tiles(H, W, 12)
    for kind, src, opacity in kinds:
        s, o = dev(src), None if opacity is None else dev(opacity)
        alone = ops.five_view_frame([(kind, 0, 0, s, o)], H, W, 1, True)
        assert int(alone[:, W:].sum()) == 0                 # the cells that no tile names are zero
        assert int(alone[:H - Z.out_rows(W), :W].sum()) == 0 and int(alone[H - Z.out_rows(W):, :W].sum()) > 0
        for r, col in ((0, 4), (2, 0), (1, 4)):
            fill = [(k, rr, cc, a, b) for rr in range(3) for (k, _, cc, a, b) in other if (rr, cc) != (r, col)]
            frame = ops.five_view_frame(fill + [(kind, r, col, s, o)], H, W, 3, True)
            assert torch.equal(frame[r * H:(r + 1) * H, col * W:(col + 1) * W], alone[:, :W]), (kind, r, col)


def test_non_finite_values_stay_in_their_column(hip_lib):
    """What a NaN or an infinity spoils is unspecified beyond its own column and channel; every other entry keeps its bound."""
    from emernerf_amd import ops
    z, _ = load_fixture()
    H, W = 37, 53
    h = Z.out_rows(W)
    rng = np.random.default_rng(3)
    src = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)
    clean = src.copy()
    src[5, 7, 1], src[20, 30, 0], src[36, 52, 2] = np.nan, np.inf, -np.inf
    keep = np.ones((W, 3), bool)
    keep[7, 1] = keep[30, 0] = keep[52, 2] = False
    v, e = Z.zoom_values("colour3", clean, None, h, z["turbo64"])
    got = ops.zoom_rows(dev(src), h).cpu().numpy()
    assert np.all(np.abs(got - v)[:, keep] <= e[:, keep])


# ------------------------------------------------------------------------------------------------------------ the refusals
def test_refusals(hip_lib):
    from emernerf_amd import _lib, ops
    from emernerf_amd import video_utils as V
    DEV = torch.device("cuda:0")
    low = [torch.rand(8, 40, 3, device=DEV) for _ in range(5)]          # h = 18 > H = 8
    with pytest.raises(ValueError, match="18"):
        list(V.compose_video_frames({"rgbs": low}, 1, ["rgbs"], 5, five_view_resize="zoom"))
    with pytest.raises(ValueError):
        ops.five_view_frame([("colour3", 0, 0, low[0], None)], 8, 40, 1, False)
    with pytest.raises(ValueError):
        ops.zoom_rows(low[0], 9)
    thin = [torch.rand(8, 4, 3, device=DEV) for _ in range(5)]          # h = 1 < 2
    with pytest.raises(ValueError):
        list(V.compose_video_frames({"rgbs": thin}, 1, ["rgbs"], 5, five_view_resize="zoom"))
    with pytest.raises(ValueError):
        ops.zoom_rows(thin[0], 1)
    ok = [torch.rand(16, 32, 3, device=DEV) for _ in range(5)]
    with pytest.raises(_lib.EmerError):    # no CPU fallback
        ops.zoom_rows(ok[0].cpu(), 14)
    with pytest.raises(_lib.EmerError):
        ops.five_view_frame([("colour3", 0, 0, ok[0].cpu(), None)], 16, 32, 1, False)
    with pytest.raises(ValueError):        # a frame of five views has five columns
        ops.five_view_frame([("colour3", 0, 5, ok[0], None)], 16, 32, 1, False)
    with pytest.raises(ValueError):
        ops.zoom_rows(torch.rand(16, 32, device=DEV), 14, "depth")       # a depth tile needs its opacity
    with pytest.raises(ValueError):
        list(V.compose_video_frames({"rgbs": ok}, 1, ["rgbs"], 5, five_view_resize="spline"))
    with pytest.raises(NotImplementedError, match="five"):               # the default still refuses five views and names the way out
        list(V.compose_video_frames({"rgbs": ok}, 1, ["rgbs"], 5))
    with pytest.raises(NotImplementedError, match="zoom"):
        V.save_videos({"rgbs": ok}, "v.mp4", 1, keys=["rgbs"], num_cams=5, writer_factory=Writers().factory)
    # "zoom" leaves groups of any other size as they are
    three = list(V.compose_video_frames({"rgbs": ok[:3]}, 1, ["rgbs"], 3, five_view_resize="zoom"))
    plain = list(V.compose_video_frames({"rgbs": ok[:3]}, 1, ["rgbs"], 3))
    np.testing.assert_array_equal(three[0][1], plain[0][1])
    out = torch.zeros(16, 96, 3, dtype=torch.uint8, device=DEV)
    tiles = [("colour3", 0, c, ok[c], None) for c in range(3)]
    assert ops.compose_frame(tiles, 16, 32, 1, 3, False, out=out) is out and torch.equal(out, ops.compose_frame(tiles, 16, 32, 1, 3, False))
    with pytest.raises(ValueError):
        ops.compose_frame(tiles, 16, 32, 1, 3, False, out=out[:, :64])
