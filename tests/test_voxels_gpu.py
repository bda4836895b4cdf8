"""The voxel-lift kernels (csrc/voxels.hip) and ``emernerf_amd.voxels`` against the restatement of tests/_voxel_ref.py -- which
tests/test_voxels_cpu.py ties to the recording of the reference's ``visualize_voxels`` -- exactly: the same voxel sets in the
same order, the same fp32 corners, the same selections.  ``lift_voxels`` is run on the recorded scene."""
import math
import types

import numpy as np
import pytest
import torch

from tests import _voxel_ref as V
from tests.golden import make_golden as G
from tests.golden import record_voxels as RV
from tests.test_voxels_cpu import KW, load_voxel_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BLOCK_BITS = 8192          # EMER_BITS_BLOCK_BITS: the voxels one compaction workgroup owns
BOX = torch.tensor([-3.0, -2.0, -1.0, 4.0, 3.0, 2.5])


def random_rays(n, seed, box=BOX):
    """End points that cover the box and leave it on every side (about a third land outside)."""
    g = torch.Generator().manual_seed(seed)
    ext = box[3:] - box[:3]
    end = box[:3] - 0.2 * ext + torch.rand(n, 3, generator=g) * 1.4 * ext
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    t = torch.rand(n, generator=g) * 5 + 0.1
    return end - d * t[:, None], d, t


def check_grid(grid, lin, box, res, what=""):
    """The grid's read-out against the restatement's linear indices: torch.equal on the int32 indices and on the fp32 corners."""
    pts, idx = grid.occupied_points(want_indices=True)
    assert pts.shape == (lin.numel(), 3) and pts.dtype == torch.float32 and idx.dtype == torch.int32 and pts.is_cuda, what
    assert torch.equal(idx.cpu().long(), V.indices_of(lin, res)), what
    assert torch.equal(pts.cpu(), V.world_corners(lin, box, res)), what
    assert torch.equal(grid.occupied_points(), pts), what


@pytest.mark.parametrize("res", [(5, 3, 7), (33, 31, 37), (41, 43, 47)])
def test_mark_and_compact_match_the_restatement(hip_lib, res):
    """(5, 3, 7): 105 voxels, a partial last word; (33, 31, 37): 37851 voxels = 4.6 compaction workgroup spans; (41, 43, 47):
    82861 voxels = 10.1 spans; set bits in every workgroup."""
    from emernerf_amd.voxels import VoxelGrid
    o, d, t = random_rays(4097, 7 + res[0])
    grid = VoxelGrid(BOX, res, DEV)
    assert grid.res == res and grid.n_voxels % 32 != 0 and grid.n_voxels % BLOCK_BITS != 0
    grid.mark(o.to(DEV), d.to(DEV), t.to(DEV))
    lin = V.mark(o, d, t, BOX, res)
    assert 0 < lin.numel() < 4097
    blocks = (grid.n_voxels + BLOCK_BITS - 1) // BLOCK_BITS
    assert blocks == {5: 1, 33: 5, 41: 11}[res[0]] and len(set((lin // BLOCK_BITS).tolist())) == blocks
    check_grid(grid, lin, BOX, res, str(res))
    # a depth filter, image-shaped inputs and a [.., 1] depth, accumulated on top of what is marked
    o2, d2, t2 = random_rays(35, 99)
    grid.mark(o2.reshape(5, 7, 3).to(DEV), d2.reshape(5, 7, 3).to(DEV), t2.reshape(5, 7, 1).to(DEV), max_depth=2.5)
    both = torch.unique(torch.cat([lin, V.mark(o2, d2, t2, BOX, res, 2.5)]))
    check_grid(grid, both, BOX, res, f"{res} second image")


@pytest.mark.parametrize("n_rays", [0, 1, 4097])
def test_ray_counts_and_many_rays_in_one_voxel(hip_lib, n_rays):
    from emernerf_amd.voxels import VoxelGrid
    res = (9, 7, 5)
    grid = VoxelGrid(BOX, res, DEV)
    g = torch.Generator().manual_seed(n_rays)
    vs = V.voxel_size(BOX, res)
    end = BOX[:3] + (torch.tensor([4.0, 3.0, 2.0]) + 0.3 + 0.4 * torch.rand(n_rays, 3, generator=g)) * vs      # all inside voxel (4, 3, 2)
    d = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    t = torch.rand(n_rays, generator=g) + 0.5
    o = end - d * t[:, None]
    grid.mark(o.to(DEV), d.to(DEV), t.to(DEV))
    lin = V.mark(o, d, t, BOX, res)
    assert lin.tolist() == [(4 * 7 + 3) * 5 + 2][:n_rays]
    check_grid(grid, lin, BOX, res)


def test_hand_made_end_points(hip_lib):
    """Voxels of 0.75 (exact in fp32) over [0, 3]^3; a zero direction makes the end point the origin itself."""
    from emernerf_amd.voxels import VoxelGrid
    box, res = torch.tensor([0.0, 0.0, 0.0, 3.0, 3.0, 3.0]), (4, 4, 4)
    eighty, nan, inf = np.float32(80.0), float("nan"), float("inf")
    rows = [  # (end point, depth, [kept linear index] or [])
        ((0.75, 1.5, 2.25), 1.0, [(1 * 4 + 2) * 4 + 3]),      # exactly on three faces: the upper voxel
        ((0.0, 0.0, 0.0), 1.0, [0]),                          # aabb_min
        ((-0.375, 0.0, 0.0), 1.0, [0]),                       # half a voxel below: kept, index 0
        ((0.0, -0.375, -0.375), 1.0, [0]),
        ((-0.75, 0.0, 0.0), 1.0, []),                         # exactly one voxel below: dropped
        ((3.0, 3.0, 3.0), 1.0, []),                           # aabb_max: dropped
        ((2.9999998, 0.0, 0.0), 1.0, [3 * 16]),
        ((1.0, 1.0, 1.0), float(eighty), []),                 # depth == max_depth: dropped
        ((1.0, 1.0, 2.0), float(np.nextafter(eighty, np.float32(0))), [(1 * 4 + 1) * 4 + 2]),
        ((1.0, 2.0, 1.0), nan, []),                           # 0 * nan
        ((nan, 1.0, 1.0), 1.0, []),
        ((inf, 1.0, 1.0), 1.0, []),
        ((1.0, -inf, 1.0), 1.0, []),
        ((1.0, 1.0, 1.0), inf, []),                           # 0 * inf
        ((3e38, 3e38, -3e38), 1.0, []),
        ((2.0, 2.0, 2.0), 1.0, [(2 * 4 + 2) * 4 + 2]),
    ]
    o = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    d = torch.zeros(len(rows), 3)
    t = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    want = torch.unique(torch.tensor(sum((r[2] for r in rows), []), dtype=torch.int64))
    assert torch.equal(V.mark(o, d, t, box, res, 80.0), want)
    grid = VoxelGrid(box, res, DEV)
    grid.mark(o.to(DEV), d.to(DEV), t.to(DEV), max_depth=80.0)
    check_grid(grid, want, box, res)
    for i, r in enumerate(rows):        # every row on its own, and every row left out: the others are unaffected
        grid.clear()
        grid.mark(o[i:i + 1].to(DEV), d[i:i + 1].to(DEV), t[i:i + 1].to(DEV), max_depth=80.0)
        check_grid(grid, torch.tensor(r[2], dtype=torch.int64), box, res, f"row {i}")
    keep = torch.tensor([math.isfinite(r[1]) and all(math.isfinite(x) for x in r[0]) for r in rows])
    assert int(keep.sum()) == len(rows) - 5
    grid.clear()
    grid.mark(o[keep].to(DEV), d[keep].to(DEV), t[keep].to(DEV), max_depth=80.0)
    check_grid(grid, want, box, res, "finite rows only")
    # a real direction: the ray runs along x and ends at 0.5 + depth
    o1, d1 = torch.tensor([[0.5, 0.1, 0.1]] * 3), torch.tensor([[1.0, 0.0, 0.0]] * 3)
    t1 = torch.tensor([0.25, 0.2, 1.0])             # 0.75: on the face, upper voxel; 0.7; 1.5: on the next face
    assert V.mark(o1, d1, t1, box, res).tolist() == [0, 16, 32]
    grid.clear()
    grid.mark(o1.to(DEV), d1.to(DEV), t1.to(DEV))
    check_grid(grid, torch.tensor([0, 16, 32]), box, res, "along x")


def test_grid_states_empty_full_and_cleared(hip_lib):
    from emernerf_amd.voxels import VoxelGrid
    res = (5, 3, 7)
    grid = VoxelGrid(BOX, res, DEV)
    pts, idx = grid.occupied_points(want_indices=True)
    assert pts.shape == (0, 3) and idx.shape == (0, 3) and pts.dtype == torch.float32 and idx.dtype == torch.int32
    assert grid.occupied_points().shape == (0, 3)
    every = torch.arange(grid.n_voxels)
    centres = BOX[:3] + (V.indices_of(every, res) + 0.5) * V.voxel_size(BOX, res)
    zeros, ones = torch.zeros(grid.n_voxels, 3), torch.ones(grid.n_voxels)
    assert torch.equal(V.mark(centres, zeros, ones, BOX, res), every)
    grid.mark(centres.to(DEV), zeros.to(DEV), ones.to(DEV))
    check_grid(grid, every, BOX, res, "full")
    assert int(grid.bits[-1]) == (1 << (grid.n_voxels % 32)) - 1          # nothing past the last voxel
    o, d, t = random_rays(300, 3)
    lin = V.mark(o, d, t, BOX, res)
    grid.clear()
    assert grid.occupied_points().shape == (0, 3)
    grid.mark(o.to(DEV), d.to(DEV), t.to(DEV))
    first = grid.occupied_points()
    check_grid(grid, lin, BOX, res, "after clear")
    grid.clear()
    grid.mark(o.to(DEV), d.to(DEV), t.to(DEV))
    assert torch.equal(grid.occupied_points(), first)


def test_two_jobs_in_one_launch_equal_two_launches(hip_lib):
    from emernerf_amd import ops
    from emernerf_amd.voxels import VoxelGrid
    o, d, t = (x.to(DEV) for x in random_rays(4097, 21))
    t2 = t * 0.7
    a, b = VoxelGrid(BOX, (33, 31, 37), DEV), VoxelGrid(BOX, 0.31, DEV)
    a2, b2 = VoxelGrid(BOX, (33, 31, 37), DEV), VoxelGrid(BOX, 0.31, DEV)
    ops.voxel_mark([a.job(o, d, t, 3.0), b.job(o, d, t2)])
    a2.mark(o, d, t, 3.0)
    b2.mark(o, d, t2)
    assert torch.equal(a.bits, a2.bits) and torch.equal(b.bits, b2.bits) and a.res != b.res
    assert int((a.bits != 0).sum()) > 0 and int((b.bits != 0).sum()) > 0
    check_grid(b, V.mark(o.cpu(), d.cpu(), t2.cpu(), BOX, b.res), BOX, b.res)


@pytest.mark.parametrize("K", [1, 3])
def test_mean_threshold_bits_and_select_rows(hip_lib, K):
    from emernerf_amd import ops
    for N in (1, 31, 32, 33, 4097):
        g = torch.Generator().manual_seed(100 * K + N)
        dens = [torch.rand(N, generator=g) for _ in range(K)]
        src = torch.randn(N, 3, generator=g)
        for thr in (0.5, -1.0, 1e9):          # some, all, none
            sel = V.mean_selector(dens, thr)
            bits = ops.mean_threshold_bits([x.to(DEV) for x in dens], thr)
            assert bits.dtype == torch.int32 and torch.equal(bits.cpu(), V.bits_of(sel)), (K, N, thr)      # bits past N are zero
            got = ops.bits_select_rows(bits, src.to(DEV))
            assert got.shape == (int(sel.sum()), 3) and torch.equal(got.cpu(), V.select_rows(sel, src)), (K, N, thr)
        assert bool(V.mean_selector(dens, -1.0).all()) and not bool(V.mean_selector(dens, 1e9).any())
        for cols in (1, 2, 4):                # the other row widths, and a [N] source
            wide = torch.randn(N, cols, generator=g)
            sel = V.mean_selector(dens, 0.5)
            bits = ops.mean_threshold_bits([x.to(DEV) for x in dens], 0.5)
            assert torch.equal(ops.bits_select_rows(bits, wide.to(DEV)).cpu(), wide[sel])
        flat = ops.bits_select_rows(bits, wide[:, 0].contiguous().to(DEV))
        assert flat.dim() == 1 and torch.equal(flat.cpu(), wide[:, 0][sel])
    # one ulp either side of the threshold.  K = 1: the value itself.  K = 3: (1 + 1) + d2 with d2 = 1 -+ 2^-22 is exact
    # (3 -+ 2^-22, one ulp of the sum either side of 3), and a third of it rounds to 1 - 2^-24 resp. 1 + 2^-23.
    if K == 1:
        thr = np.float32(0.1)
        dens = [torch.tensor([float(np.nextafter(thr, np.float32(-1))), float(thr), float(np.nextafter(thr, np.float32(1)))] * 11, dtype=torch.float32)]
        thr = float(thr)
    else:
        thr, e = 1.0, 2.0 ** -22
        dens = [torch.ones(33), torch.ones(33), torch.tensor([1.0 - e, 1.0, 1.0 + e] * 11)]
    want = torch.tensor([False, False, True] * 11)
    assert torch.equal(V.mean_selector(dens, thr), want)
    bits = ops.mean_threshold_bits([x.to(DEV) for x in dens], thr)
    assert torch.equal(bits.cpu(), V.bits_of(want))
    nan = [x.clone() for x in dens]
    nan[0][2] = float("nan")
    want_nan = want.clone()
    want_nan[2] = False
    assert torch.equal(ops.mean_threshold_bits([x.to(DEV) for x in nan], thr).cpu(), V.bits_of(want_nan))


def test_recorded_selection(hip_lib):
    """The recorded candidate points and per-point densities: the kernels' selection is the recording's."""
    from emernerf_amd import ops
    z, *_ = load_voxel_case()
    t = lambda k: torch.from_numpy(z[k]).to(DEV)  # noqa: E731
    kept = ops.bits_select_rows(ops.mean_threshold_bits([t(f"static/density/{k}") for k in range(3)], 0.5), t("static/candidates"))
    assert torch.equal(kept, t("coords"))
    kept = ops.bits_select_rows(ops.mean_threshold_bits([t("dynamic/0/density")], 0.1), t("dynamic/0/candidates"))
    assert torch.equal(kept, t("dynamic_coords/0"))


def test_wrappers_reject_bad_arguments(hip_lib):
    from emernerf_amd import ops
    from emernerf_amd._lib import EmerError
    from emernerf_amd.voxels import VoxelGrid
    grid = VoxelGrid(BOX, (5, 3, 7), DEV)
    o, d, t = (x.to(DEV) for x in random_rays(8, 1))
    with pytest.raises(EmerError):
        grid.mark(o.cpu(), d, t)
    with pytest.raises(EmerError):
        grid.mark(o, d, t[:7])
    with pytest.raises(EmerError):
        ops.voxel_mark([(o, d, t, math.inf, (0, 0, 0), (1, 1, 1), (5, 3, 7), grid.bits[:-1])])
    with pytest.raises(EmerError):
        ops.voxel_mark([(o, d, t, math.inf, (0, 0, 0), (1, 1, 1), (5, 3, 7), grid.bits.float())])
    with pytest.raises(EmerError):
        ops.voxel_mark([(o, d, t, math.inf, (0, 0, 0), (0, 1, 1), (5, 3, 7), grid.bits)])      # a zero voxel size (the library's check)
    with pytest.raises(EmerError):
        ops.mean_threshold_bits([t] * 9, 0.5)
    with pytest.raises(EmerError):
        ops.mean_threshold_bits([t, t[:7]], 0.5)
    with pytest.raises(EmerError):
        ops.bits_select_rows(ops.mean_threshold_bits([t], 0.5), torch.zeros(8, 5, device=DEV))
    with pytest.raises(EmerError):
        ops.bits_select_rows(ops.mean_threshold_bits([t], 0.5), torch.zeros(40, 3, device=DEV))
    assert grid.occupied_points().shape == (0, 3)          # nothing was marked on the way


# ------------------------------------------------------------------------------------------------------------- the loop
def _recorded_scene():
    from emernerf_amd import radiance_field
    from emernerf_amd.prop_net import PropNetEstimator
    z, rec_rendered, box, res, dres = load_voxel_case()
    model, props = RV.build_scene_models(radiance_field, int(z["model_seed"]), int(z["table_seed"]), DEV)
    for k, v in RV.state_digests(model, props).items():       # the seeded construction is the recorded model
        np.testing.assert_allclose(v, z[k], rtol=1e-9, atol=1e-12, err_msg=f"{k}: the rebuilt model is not the recorded one")
    est = PropNetEstimator(None, None).to(DEV)
    images = [{k: v.to(DEV) for k, v in d.items()} for d in RV.voxel_images(KW["seed"], KW["n_images"], KW["hw"])]
    dataset = types.SimpleNamespace(full_pixel_set=G.GoldenSplit(images), num_cams=KW["num_cams"],
                                    pixel_source=types.SimpleNamespace(unique_normalized_timestamps=RV.unique_timestamps(KW["n_images"], KW["num_cams"])))
    return z, rec_rendered, box, res, dres, model, props, est, dataset


def test_lift_voxels_on_the_recorded_scene(hip_lib):
    from emernerf_amd import voxels
    z, rec_rendered, box, res, dres, model, props, est, dataset = _recorded_scene()
    cfg = RV.voxel_cfg(KW["vis_voxel_size"])
    pca = tuple(torch.from_numpy(z["pca/" + k]) for k in ("mat", "lo", "hi"))
    default = voxels._default_render_func(cfg, model, est, props)
    rendered, calls = [], []

    def render_func(data_dict, lidar):
        out = default(data_dict, lidar)
        calls.append(lidar)
        if lidar:
            rendered.append({"origins": data_dict["lidar_origins"].cpu(), "viewdirs": data_dict["lidar_viewdirs"].cpu(),
                             **{k: out[k].cpu() for k in ("depth", "static_depth", "dynamic_depth")}})
        else:
            assert "dino_pe_free" in out
        return out
    model.train()
    out = voxels.lift_voxels(cfg, model, est, props, dataset, is_dynamic=True, pca=pca, render_func=render_func)
    assert model.training and torch.is_grad_enabled()          # the modes are put back
    # the first num_cams images are rendered in full as well, every image in forced-lidar mode
    assert calls == [False, True, False, True] + [True] * 5 and len(rendered) == KW["n_images"]
    assert set(out) == {"coords", "colors", "dynamic_coords", "dynamic_colors", "vis_aabb", "pca"}
    assert out["vis_aabb"] == z["vis_aabb"].tolist() and all(torch.equal(a.cpu(), b) for a, b in zip(out["pca"], pca))
    assert out["coords"].is_cuda and out["colors"].is_cuda and len(out["dynamic_coords"]) == len(out["dynamic_colors"]) == 1

    # ---- against the restatement applied to the depths it rendered itself: points exactly, colours to 1e-6
    static, dyn = V.lift(rendered, box, KW["vis_voxel_size"], KW["num_cams"], True)
    cand = V.world_corners(static, box, res)
    with torch.no_grad():
        model.eval()
        dens = [p(cand.to(DEV))["density"].squeeze(-1).cpu() for p in props]
        dens.append(model.forward(cand.to(DEV), query_feature_head=False)["density"].reshape(-1).cpu())
        sel = V.mean_selector(dens, 0.5)
        kept = V.select_rows(sel, cand)
        feats = model.forward(kept.to(DEV), query_feature_head=True, query_pe_head=False)["dino_feat"].cpu()
        dcand = V.world_corners(dyn[0], box, dres)
        ts = dataset.pixel_source.unique_normalized_timestamps[0].to(DEV)
        dd = model.forward(dcand.to(DEV), data_dict={"normed_timestamps": ts.repeat(dcand.shape[0], 1)}, query_feature_head=False)
        dsel = V.mean_selector([dd["dynamic_density"].reshape(-1).cpu()], 0.1)
        dkept = V.select_rows(dsel, dcand)
        dfeats = model.forward(dkept.to(DEV), data_dict={"normed_timestamps": ts.repeat(dkept.shape[0], 1)}, query_feature_head=True,
                               query_pe_head=False)["dynamic_dino_feat"].cpu()
    assert 0 < kept.shape[0] < cand.shape[0] and 0 < dkept.shape[0] < dcand.shape[0]
    assert torch.equal(out["coords"].cpu(), kept)
    assert torch.equal(out["dynamic_coords"][0].cpu(), dkept)
    for name, got, want in (("colors", out["colors"], V.colours(feats, *pca)), ("dynamic_colors", out["dynamic_colors"][0], V.colours(dfeats, *pca))):
        err = float((got.cpu() - want).abs().max())
        print(f"{name}: max |kernel - restatement| = {err:.3e} over {tuple(want.shape)}")
        assert got.shape == want.shape and err <= 1e-6, (name, err)

    # ---- against the recording: depths within the tolerance of test_golden_gpu's render_pixels depths; the voxel sets may differ
    # only in voxels that hold a recorded end point within that tolerance of a face, at most 10 % of the recorded voxels
    for i, (mine, rec) in enumerate(zip(rendered, rec_rendered)):
        for k in ("depth", "static_depth", "dynamic_depth"):
            want = rec[k].double()
            err = (mine[k].double() - want).abs()
            bound = RV.DEPTH_ATOL * max(float(want.abs().max()), 1.0) + RV.DEPTH_RTOL * want.abs()
            print(f"image {i} {k}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (i, k, float(err.max()))
    rec_static, rec_dyn = V.lift(rec_rendered, box, KW["vis_voxel_size"], KW["num_cams"], True)
    groups = V.groups(KW["n_images"], KW["num_cams"])
    cases = [("static", static, rec_static, rec_rendered, "static_depth", res, 80.0)]
    cases += [(f"dynamic group {j}", dyn[j], rec_dyn[j], [rec_rendered[i] for i in g], "dynamic_depth", dres, math.inf) for j, g in enumerate(groups)]
    allowed = {}
    for name, mine, rec, rr, key, r3, max_depth in cases:
        tols = [RV.depth_tolerance(r[key]) for r in rr]
        allowed[name] = set(V.face_allowance(rr, key, tols, box, r3, max_depth).tolist())
        diff = set(mine.tolist()) ^ set(rec.tolist())
        print(f"{name}: {rec.numel()} recorded voxels, {len(diff)} differ, {len(allowed[name])} may")
        assert diff <= allowed[name], (name, sorted(diff - allowed[name]))
        assert len(diff) <= 0.1 * rec.numel(), (name, len(diff), rec.numel())
    # the kept points: the recording's, but for the voxels above
    for name, lin, selector, rec_pts, r3 in (("static", static, sel, z["coords"], res), ("dynamic group 0", dyn[0], dsel, z["dynamic_coords/0"], dres)):
        rec_lin = {tuple(p) for p in rec_pts.tolist()}
        mine_pts = {tuple(p) for p in V.world_corners(lin[selector], box, r3).tolist()}
        shaky = {tuple(p) for p in V.world_corners(torch.tensor(sorted(allowed[name]), dtype=torch.int64), box, r3).tolist()}
        assert (mine_pts ^ rec_lin) <= shaky, (name, sorted(mine_pts ^ rec_lin))


def test_lift_voxels_static_model_without_feature_head(hip_lib):
    """is_dynamic=False on a model with no feature head: ``depth`` feeds the static grid, no dynamic entries, colours are None."""
    from emernerf_amd import voxels
    from emernerf_amd.prop_net import PropNetEstimator
    from emernerf_amd.radiance_field import build_density_field, build_radiance_field_from_cfg
    torch.manual_seed(3)
    model = build_radiance_field_from_cfg(G.model_cfg("static"), verbose=False)
    model.set_aabb(G.AABB)
    props = [build_density_field(aabb=G.AABB, unbounded=True, **kw) for kw in G.PROP_KW]
    G.randomize_tables({"model/": model, **{f"prop{i}/": p for i, p in enumerate(props)}}, 4)
    with torch.no_grad():
        for lin in [p.base_mlp[-1] for p in props] + [model.base_mlp[-1]]:
            lin.bias[0] += 1.0          # densities around exp(0): every candidate passes 0.5
    for m in [model, *props]:
        m.to(DEV)
    est = PropNetEstimator(None, None).to(DEV)
    images = []
    for i in range(3):
        d = G.make_rays(35, 50 + i, 10, 1, (5, 7))
        d.pop("features")
        images.append({k: v.to(DEV) for k, v in d.items()})
    dataset = types.SimpleNamespace(full_pixel_set=G.GoldenSplit(images), num_cams=1, pixel_source=None)
    cfg = RV.voxel_cfg(4.0)
    rendered = []
    default = voxels._default_render_func(cfg, model, est, props)

    def render_func(data_dict, lidar):
        out = default(data_dict, lidar)
        if lidar:
            rendered.append({"origins": data_dict["lidar_origins"].cpu(), "viewdirs": data_dict["lidar_viewdirs"].cpu(), "depth": out["depth"].cpu()})
        return out
    out = voxels.lift_voxels(cfg, model, est, props, dataset, is_dynamic=False, render_func=render_func)
    assert out["colors"] is None and out["dynamic_coords"] is None and out["dynamic_colors"] is None and out["pca"] is None
    box = V.vis_aabb(G.AABB)
    static, _ = V.lift(rendered, box, 4.0, 1, False)
    cand = V.world_corners(static, box, V.resolution(box, 4.0))
    with torch.no_grad():
        dens = [p(cand.to(DEV))["density"].squeeze(-1).cpu() for p in props] + [model.forward(cand.to(DEV), query_feature_head=False)["density"].reshape(-1).cpu()]
    kept = V.select_rows(V.mean_selector(dens, 0.5), cand)
    assert kept.shape[0] > 0 and torch.equal(out["coords"].cpu(), kept)
