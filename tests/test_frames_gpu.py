"""The video-frame kernel (csrc/frames.hip), ``ops.compose_frame`` / ``depth_colours`` and ``video_utils.compose_video_frames`` /
``save_videos`` on the GPU: against the recording of the reference's own ``save_concatenated_videos`` /
``save_seperate_videos`` (tests/golden/video_frames.npz) and against the numpy restatement of tests/_frame_ref.py on seeded
images.  Non-depth pixels must match bit for bit; a depth pixel must lie in its set of acceptable table rows (the device's
logf against numpy's fp32 log: tests/_frame_ref.py), and no more pixels may take a second choice than have one."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _frame_ref as R
from tests.test_frames_cpu import case_results, load_fixture, recorded_frames

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assert_frame(got, three, what):
    ok, second, ambiguous = R.compare(got, three)
    assert ok, f"{what}: {int(np.sum(np.any(got != three[0], axis=-1)))} pixels differ from the restatement, some by more than the logarithm allows"
    assert second <= ambiguous, f"{what}: {second} pixels took a second choice, {ambiguous} have one"
    return second


def plan_tiles(plan, i, num_cams, to_dev=True):
    """The tiles of frame ``i`` of a frame plan, for ops.compose_frame (device) or R.compose (numpy)."""
    conv = dev if to_dev else np.asarray
    tiles = []
    for r, (_, kind, images, opacities) in enumerate(plan):
        for c, x in enumerate(images[i * num_cams:(i + 1) * num_cams]):
            tiles.append((kind, r, c, conv(x), None if opacities is None else conv(opacities[i * num_cams + c])))
    return tiles


# ------------------------------------------------------------------------------------------------- against the recording
@pytest.mark.parametrize("name", ["A_cat", "A_plain", "B_cat"])
def test_compose_frame_matches_recording_with_both_flags(hip_lib, name):
    """The merged frames of the recording from ``ops.compose_frame``: with the recorded scaling (fp64 where a depth row is in the
    frame, else fp32) against the recording, with both flags against the restatement."""
    from emernerf_amd import ops
    z, meta = load_fixture()
    c = meta["cases"][name]
    res = case_results(z, c)
    plan = R.frame_plan(res, c["keys"], False)
    recorded_flag = any(kind == "depth" for _, kind, _, _ in plan)
    assert recorded_flag == (name != "A_plain")
    rec = recorded_frames(z, name)
    for i in range(c["num_timestamps"]):
        tiles = plan_tiles(plan, i, c["num_cams"])
        H, W = tiles[0][3].shape[:2]
        for flag in (False, True):
            got = ops.compose_frame(tiles, H, W, len(plan), c["num_cams"], flag)
            assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (len(plan) * H, c["num_cams"] * W, 3)
            got = got.cpu().numpy()
            three = R.compose(plan_tiles(plan, i, c["num_cams"], False), H, W, len(plan), c["num_cams"], flag, z["turbo8"])
            assert_frame(got, three, f"{name} frame {i} fp64={flag}")
            if flag == recorded_flag:
                assert_frame(got, (rec[i], three[1], three[2]), f"{name} frame {i} vs the recording")
                depth_rows = np.zeros(got.shape[0], bool)
                for r, (_, kind, _, _) in enumerate(plan):
                    depth_rows[r * H:(r + 1) * H] = kind == "depth"
                np.testing.assert_array_equal(got[~depth_rows], rec[i][~depth_rows])      # colour, mask and sky rows: bit for bit


class Writers:
    """A recording ``writer_factory`` / ``image_writer``."""

    def __init__(self):
        self.opened, self.frames, self.images, self.closed = [], [], [], []

    def factory(self, path, **kw):
        rec = self
        rec.opened.append((path, kw))

        class W:
            def append_data(self, frame):
                rec.frames.append((path, frame))

            def close(self):
                rec.closed.append(path)
        return W()

    def imwrite(self, path, image):
        self.images.append((path, image))


@pytest.mark.parametrize("source", ["numpy", "device"])
@pytest.mark.parametrize("name", ["A_cat", "A_plain", "A_sep", "B_cat", "B_sep"])
def test_save_videos_matches_recording(hip_lib, name, source, tmp_path, monkeypatch):
    """``save_videos`` with a recording writer hands over the recorded frames in the recorded order and returns the recorded
    frame; ``compose_video_frames`` yields the same frames.  From numpy lists and from device tensors."""
    from emernerf_amd import video_utils as V
    z, meta = load_fixture()
    c = meta["cases"][name]
    res = case_results(z, c)
    if source == "device":
        res = {k: [dev(a) for a in v] for k, v in res.items()}
    mine = R.video_frames(case_results(z, c), c["num_timestamps"], c["keys"], c["num_cams"], c["separate"], z["turbo8"])
    rec = recorded_frames(z, name)
    tags = [str(t) for t in z[name + "/tags"]]
    monkeypatch.chdir(tmp_path)          # save_images makes its directories next to save_pth
    w = Writers()
    ret = V.save_videos(res, c["save_pth"], c["num_timestamps"], keys=list(c["keys"]), num_cams=c["num_cams"],
                        save_seperate_video=c["separate"], save_images=c["separate"], verbose=False, writer_factory=w.factory,
                        image_writer=w.imwrite)
    assert [p for p, _ in w.frames] == tags
    for (path, f), want, (tag, three) in zip(w.frames, rec, mine):
        assert isinstance(f, np.ndarray) and f.dtype == np.uint8
        assert_frame(f, (want, three[1], three[2]), f"{name} {tag} ({source})")
    # the writers: the recorded ones that received frames (none is opened for a skipped key), with the recorded arguments
    recorded_writers = [tuple(json.loads(str(s))) for s in z[name + "/writers"]]
    used = [(p, kw) for p, kw in recorded_writers if p in tags]
    assert [(p, kw) for p, kw in w.opened] == used and w.closed == [p for p, _ in used]
    mid = 0 if c["num_timestamps"] == 1 else c["num_timestamps"] // 2
    returned = {k[len(name) + len("/return/"):]: v for k, v in z.items() if k.startswith(name + "/return/")}
    assert set(ret) == set(returned)
    by_tag = {tag: three for tag, three in mine}
    for k, f in ret.items():
        three = by_tag[(k, mid)] if c["separate"] else by_tag[(mid,)]
        assert_frame(f, (returned[k], three[1], three[2]), f"{name}: returned {k}")
    if c["separate"]:
        names = [str(s) for s in z[name + "/image_names"]]
        assert [p for p, _ in w.images] == names
        n = 0
        for tag, three in mine:
            W = three[0].shape[1] // c["num_cams"]
            for j in range(c["num_cams"]):
                cut = tuple(t[:, j * W:(j + 1) * W] for t in three)
                assert_frame(w.images[n][1], (z[f"{name}/image/{n}"], cut[1], cut[2]), names[n])
                n += 1
    # the generator on its own
    frames = list(V.compose_video_frames(res, c["num_timestamps"], list(c["keys"]), c["num_cams"], separate=c["separate"]))
    assert [f[:-1] for f in frames] == [tag for tag, _ in mine]
    for f, (path, g) in zip(frames, w.frames):
        np.testing.assert_array_equal(f[-1], g)


# ---------------------------------------------------------------------------------------- seeded images vs the restatement
DEPTH_EDGE = np.array([0.0, -1.0, -1e-6, np.inf, np.nan, 4.0, 120.0, 3.0, 121.0, 1e-30, 3e38], dtype=np.float32)
OPACITY_EDGE = np.array([0.0, 1.0, 1 + 1e-7, 1.5, np.nan, -0.5, np.inf], dtype=np.float32)


def seeded_tiles(H, W, cams, seed):
    """Four rows (colour, mask, sky, depth) of ``cams`` seeded [H, W] images, as numpy tiles."""
    rng = np.random.default_rng(seed)
    n = H * W
    tiles = []
    for c in range(cams):
        col = rng.uniform(-0.2, 1.2, (H, W, 3)).astype(np.float32)
        col.reshape(-1)[rng.permutation(3 * n)[:6]] = [np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0]
        mask = np.where(rng.uniform(0, 1, (H, W)) < 0.5, rng.uniform(0, 1, (H, W)), (rng.uniform(0, 1, (H, W)) < 0.5)).astype(np.float32)
        opa = rng.uniform(-0.1, 1.1, (H, W)).astype(np.float32)
        depth = np.exp(rng.uniform(np.log(1.0), np.log(300.0), n)).astype(np.float32)
        dop = np.clip(rng.uniform(-0.2, 1.2, n), 0, 1).astype(np.float32)
        pairs = np.array([(d, o) for d in DEPTH_EDGE for o in OPACITY_EDGE], dtype=np.float32)
        where = rng.permutation(n)[:len(pairs)]
        depth[where], dop[where] = pairs[:len(where), 0], pairs[:len(where), 1]
        tiles += [("colour3", 0, c, col, None), ("grey1", 1, c, mask, None), ("one_minus_grey1", 2, c, opa, None),
                  ("depth", 3, c, depth.reshape(H, W), dop.reshape(H, W))]
    return tiles


def to_device(tiles, offset=0):
    """The tiles on the device; ``offset`` > 0: every source is a view that starts ``offset`` floats into its storage."""
    def put(a):
        if a is None:
            return None
        if offset == 0:
            return dev(a)
        buf = torch.empty(a.size + offset, dtype=torch.float32, device=DEV)
        view = buf[offset:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.storage_offset() == offset and view.is_contiguous()
        return view
    return [(kind, r, c, put(src), put(opacity)) for kind, r, c, src, opacity in tiles]


@pytest.mark.parametrize("H,W,cams", [(37, 53, 1), (37, 53, 2), (8, 16, 3), (8, 16, 6)])
def test_seeded_frames_match_restatement_on_every_path(hip_lib, H, W, cams):
    """37 x 53 (odd sizes, several workgroups: byte stores, scalar loads) and 8 x 16 (dword stores, 16-byte loads); the same
    data behind a view with an odd storage offset takes the scalar loads and must give the same bytes; both scaling flags."""
    from emernerf_amd import ops
    tiles = seeded_tiles(H, W, cams, 100 * H + cams)
    z, _ = load_fixture()
    for flag in (False, True):
        three = R.compose(tiles, H, W, 4, cams, flag, z["turbo8"])
        got = ops.compose_frame(to_device(tiles), H, W, 4, cams, flag)
        assert_frame(got.cpu().numpy(), three, f"{H} x {W} x {cams} fp64={flag}")
        np.testing.assert_array_equal(got.cpu().numpy()[:3 * H], three[0][:3 * H])
        for offset in (1, 3):
            view = ops.compose_frame(to_device(tiles, offset), H, W, 4, cams, flag)
            assert torch.equal(view, got), f"a view {offset} floats into its storage gives other bytes"
    kind, _, _, d, o = tiles[3]
    one = ops.depth_colours(dev(d), dev(o))
    assert tuple(one.shape) == (H, W, 3) and torch.equal(one, got[3 * H:, :W])


def test_frame_with_more_work_items_than_the_grid_holds(hip_lib):
    """4 tiles of 520 x 1012: 526 240 groups of four pixels, more than the 2048 x 256 lanes of the capped grid, so the lanes
    stride over the frame; every kind, against the restatement."""
    from emernerf_amd import ops
    H, W = 520, 1012
    assert (W // 4) * H * 4 > 2048 * 256
    tiles = seeded_tiles(H, W, 1, 5)
    z, _ = load_fixture()
    got = ops.compose_frame(to_device(tiles), H, W, 4, 1, True).cpu().numpy()
    three = R.compose(tiles, H, W, 4, 1, True, z["turbo8"])
    assert_frame(got, three, "520 x 1012")
    np.testing.assert_array_equal(got[:3 * H], three[0][:3 * H])


# ------------------------------------------------------------------------------------------------------------ independence
def test_a_tiles_bytes_do_not_depend_on_its_cell_or_its_neighbours(hip_lib):
    from emernerf_amd import ops
    H, W = 9, 12
    tiles = seeded_tiles(H, W, 1, 7)
    other = to_device(seeded_tiles(H, W, 1, 8))
    for kind, _, _, src, opacity in to_device(tiles):
        alone = ops.compose_frame([(kind, 0, 0, src, opacity)], H, W, 1, 1, True)
        for r, c in ((0, 0), (2, 2)):
            fill = [(k, rr, cc, s, o) for (k, _, _, s, o), (rr, cc) in zip(other * 3, [(a, b) for a in range(3) for b in range(3) if (a, b) != (r, c)])]
            frame = ops.compose_frame(fill + [(kind, r, c, src, opacity)], H, W, 3, 3, True)
            assert torch.equal(frame[r * H:(r + 1) * H, c * W:(c + 1) * W], alone), (kind, r, c)
    # a frame that names only some cells leaves the others zero
    part = ops.compose_frame([(tiles[0][0], 1, 1, dev(tiles[0][3]), None)], H, W, 2, 2, False)
    assert int(part[:H].sum()) == 0 and int(part[:, :W].sum()) == 0 and int(part[H:, W:].sum()) > 0


def test_more_tiles_than_one_launch_takes(hip_lib):
    """rows x cams > FRAME_TILES_MAX: several launches over disjoint tiles; every cell equals the tile composed alone."""
    from emernerf_amd import ops
    H, W, rows, cams = 3, 5, 8, 7
    assert rows * cams > ops.FRAME_TILES_MAX
    base = to_device(seeded_tiles(H, W, 1, 21))
    tiles = [(*base[(r + c) % 4][:1], r, c, *base[(r + c) % 4][3:]) for r in range(rows) for c in range(cams)]
    frame = ops.compose_frame(tiles, H, W, rows, cams, True)
    alone = [ops.compose_frame([(b[0], 0, 0, b[3], b[4])], H, W, 1, 1, True) for b in base]
    for r in range(rows):
        for c in range(cams):
            assert torch.equal(frame[r * H:(r + 1) * H, c * W:(c + 1) * W], alone[(r + c) % 4]), (r, c)


# ------------------------------------------------------------------------------------------------------------ the refusals
def test_refusals(hip_lib):
    from emernerf_amd import _lib, ops
    from emernerf_amd import video_utils as V
    H, W = 4, 8
    rgb = [torch.rand(H, W, 3, device=DEV) for _ in range(5)]
    d = [torch.rand(H, W, device=DEV) * 50 + 1 for _ in range(5)]
    o = [torch.rand(H, W, device=DEV) for _ in range(5)]
    for kw in (dict(lo=None), dict(hi=None)):
        with pytest.raises(NotImplementedError, match="percentile"):
            ops.depth_colours(d[0], o[0], **kw)
        with pytest.raises(NotImplementedError, match="percentile"):
            ops.compose_frame([("depth", 0, 0, d[0], o[0])], H, W, 1, 1, False, **kw)
    res = {"rgbs": rgb, "depths": d, "opacities": o, "static_depths": d}
    with pytest.raises(NotImplementedError, match="five"):
        list(V.compose_video_frames(res, 1, ["rgbs", "depths"], 5))
    w = Writers()
    with pytest.raises(NotImplementedError, match="five"):
        V.save_videos(res, "v.mp4", 1, keys=["rgbs"], num_cams=5, writer_factory=w.factory)
    frames = list(V.compose_video_frames(res, 1, ["rgbs", "depths"], 5, five_view_resize=False))     # tiled unresized
    assert len(frames) == 1 and frames[0][1].shape == (2 * H, 5 * W, 3)
    with pytest.raises(KeyError):          # separate mode: no opacity list for static_depths
        list(V.compose_video_frames(res, 1, ["static_depths"], 1, separate=True))
    assert [f[0] for f in V.compose_video_frames(res, 1, ["static_depths", "rgbs"], 1)] == [0]       # merged mode: skipped
    with pytest.raises(ValueError):        # sizes differ within one frame
        list(V.compose_video_frames({"rgbs": [rgb[0], torch.rand(H, W + 4, 3, device=DEV)]}, 1, ["rgbs"], 2))
    with pytest.raises(ValueError):
        list(V.compose_video_frames({"rgbs": rgb, "gt_rgbs": [torch.rand(H + 1, W, 3, device=DEV)] * 5}, 1, ["rgbs", "gt_rgbs"], 1))
    with pytest.raises(ValueError):        # a colour key whose images have one channel
        list(V.compose_video_frames({"opacities": o}, 1, ["opacities"], 1))
    with pytest.raises(ValueError):        # ... or four
        list(V.compose_video_frames({"rgbs": [torch.rand(H, W, 4, device=DEV)]}, 1, ["rgbs"], 1))
    with pytest.raises(ValueError):
        ops.compose_frame([("colour3", 0, 0, d[0], None)], H, W, 1, 1, False)
    with pytest.raises(ValueError):
        ops.compose_frame([("depth", 0, 0, d[0], None)], H, W, 1, 1, False)
    with pytest.raises(ValueError):
        ops.compose_frame([("colour3", 1, 0, rgb[0], None)], H, W, 1, 1, False)
    with pytest.raises(_lib.EmerError):    # no CPU fallback
        ops.compose_frame([("colour3", 0, 0, rgb[0].cpu(), None)], H, W, 1, 1, False)


# ------------------------------------------------------------------------------------------- the render loop's device lists
def test_render_pixels_device_lists_feed_save_videos(hip_lib):
    """``render_pixels(..., to_host=False)`` on the static case of tests/golden/render_pixels_static.npz: the lists hold device
    tensors bitwise equal to the host lists, the scalars agree, and ``save_videos`` gives the same frames from either."""
    from emernerf_amd import video_utils as V
    from emernerf_amd.prop_net import PropNetEstimator
    from emernerf_amd.radiance_field import build_density_field, build_radiance_field_from_cfg
    from tests.golden import make_golden as G
    from tests.test_golden_gpu import _load
    case = "render_pixels_static"
    gold = _load(case)
    cfg = G.model_cfg(G.RENDER_PIXELS_CASES[case]["kind"])
    torch.manual_seed(0)
    model = build_radiance_field_from_cfg(cfg, verbose=False)
    props = [build_density_field(aabb=G.AABB, unbounded=True, **k) for k in G.PROP_KW]
    seed = int(gold["table_seed"])
    for prefix, m in [("model/", model)] + [(f"prop{i}/", p) for i, p in enumerate(props)]:
        sd = {k: (G.table_values(prefix + k, v.numel(), seed) if k.endswith("tcnn_encoding.params")
                  else torch.from_numpy(gold["state/" + prefix + k])) for k, v in m.state_dict().items()}
        m.load_state_dict(sd)
        m.to(DEV)
    model.time_diff = 1 / cfg.num_train_timesteps
    est = PropNetEstimator(None, None).to(DEV)
    n_img = len({k.split("/")[0] for k in gold if k.startswith("image")})
    images = [{k[len(f"image{i}/"):]: torch.from_numpy(v).to(DEV) for k, v in gold.items() if k.startswith(f"image{i}/")} for i in range(n_img)]
    rcfg = G.render_cfg([24, 16], 16, chunk=25)
    outs = {}
    for to_host in (True, False):
        outs[to_host] = V.render_pixels(rcfg, model, est, G.GoldenSplit(images), proposal_networks=props, compute_metrics=True,
                                        return_decomposition=True, to_host=to_host)
    on_host, on_dev = outs[True], outs[False]
    assert set(on_host) == set(on_dev)
    lists = [k for k, v in on_host.items() if isinstance(v, list)]
    assert {"rgbs", "gt_rgbs", "depths", "opacities"} <= set(lists)
    for k in lists:
        assert len(on_dev[k]) == len(on_host[k]), k
        for a, b in zip(on_dev[k], on_host[k]):
            assert isinstance(a, torch.Tensor) and a.is_cuda and isinstance(b, np.ndarray), k
            assert tuple(a.shape) == b.shape and a.cpu().numpy().dtype == b.dtype, k
            np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=k)
    for k in ("psnr", "ssim", "masked_psnr"):
        assert on_dev[k] == on_host[k], k
    keys = [k for k in ("gt_rgbs", "rgbs", "depths", "gt_sky_masks", "sky_masks") if k == "sky_masks" or len(on_host.get(k, [])) > 0]
    assert len(keys) >= 4
    frames = {}
    for to_host in (True, False):
        w = Writers()
        ret = V.save_videos(outs[to_host], "eval.mp4", 1, keys=keys, num_cams=n_img, verbose=False, writer_factory=w.factory)
        assert len(w.frames) == 1 and w.frames[0][1] is ret["concatenated_frame"]
        frames[to_host] = ret["concatenated_frame"]
    H, W = on_host["rgbs"][0].shape[:2]
    assert frames[True].shape == (len(keys) * H, n_img * W, 3) and frames[True].dtype == np.uint8
    np.testing.assert_array_equal(frames[True], frames[False])
    z, _ = load_fixture()
    want = R.video_frames(on_host, 1, keys, n_img, False, z["turbo8"])
    assert_frame(frames[True], want[0][1], "the eval loop's frame")
