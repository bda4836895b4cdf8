"""The restatement of the voxel lift (tests/_voxel_ref.py) against the recording of the reference's ``visualize_voxels``
(tests/golden/voxels.npz, record_voxels.py): fed with the recorded depths, rays, densities and PCA it reproduces the recorded
voxel sets, their order and the selected points exactly and the colours to 1e-6.  No GPU: the kernels are held to the same
restatement in tests/test_voxels_gpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import _voxel_ref as V
from tests.golden import make_golden as G
from tests.golden import record_voxels as RV

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxels.npz")
KW = RV.VOXELS


def load_voxel_case():
    """(fixture, per-image rendered dicts as CPU tensors, vis aabb, static resolution, dynamic resolution)."""
    z = np.load(GOLDEN)
    rendered = [{k: torch.from_numpy(z[f"image{i}/{k}"]) for k in ("origins", "viewdirs", "depth", "static_depth", "dynamic_depth")}
                for i in range(KW["n_images"])]
    box = torch.from_numpy(z["vis_aabb"])
    return z, rendered, box, V.resolution(box, KW["vis_voxel_size"]), V.resolution(box, KW["vis_voxel_size"], 0.8)


def test_fixture_is_small_and_holds_the_rays_it_was_recorded_on():
    assert os.path.getsize(GOLDEN) <= 200_000
    z, rendered, box, res, dres = load_voxel_case()
    images = RV.voxel_images(KW["seed"], KW["n_images"], KW["hw"])
    for r, d in zip(rendered, images):
        assert torch.equal(r["origins"], d["origins"]) and torch.equal(r["viewdirs"], d["viewdirs"])
        assert r["static_depth"].shape == (*KW["hw"], 1)
    assert res == (26, 21, 6) and dres == (21, 17, 5)
    assert 1000 <= res[0] * res[1] * res[2] <= 10000


def test_vis_aabb_keeps_the_reference_slice():
    z = np.load(GOLDEN)
    from emernerf_amd.voxels import vis_aabb
    for fn in (V.vis_aabb, vis_aabb):
        got = fn(torch.tensor(G.AABB))
        assert got.tolist() == z["vis_aabb"].tolist() == [-20.0, -41.0, -1.0, 81.0, 41.0, 21.0]      # x_min is not expanded
        assert torch.equal(fn(torch.tensor(G.AABB).reshape(2, 3)), got)


def test_voxel_grid_host_side_matches_the_restatement():
    from emernerf_amd.voxels import VoxelGrid
    z, _, box, res, dres = load_voxel_case()
    g = VoxelGrid(box, KW["vis_voxel_size"], "cpu")
    assert g.res == res and torch.equal(g.voxel_size, V.voxel_size(box, res)) and g.bits.numel() == (g.n_voxels + 31) // 32
    d = VoxelGrid(box, dres, "cpu")
    assert d.res == dres and torch.equal(d.voxel_size, V.voxel_size(box, dres))
    for size in (0.3, 0.15):     # the shipped box at the default voxel sizes: ceil of an fp32 quotient
        b = V.vis_aabb(G.AABB)
        assert VoxelGrid(b, size, "cpu").res == V.resolution(b, size)


def test_restatement_reproduces_the_recorded_candidates_in_order():
    z, rendered, box, res, dres = load_voxel_case()
    static, dyn = V.lift(rendered, box, KW["vis_voxel_size"], KW["num_cams"], True)
    assert len(dyn) == 3 and V.groups(7, 2) == [[0, 1, 2], [3, 4], [5, 6]]
    assert torch.equal(V.world_corners(static, box, res), torch.from_numpy(z["static/candidates"]))
    assert torch.equal(V.world_corners(dyn[0], box, dres), torch.from_numpy(z["dynamic/0/candidates"]))
    assert float(z["dynamic/0/timestamp"].reshape(-1)[0]) == float(RV.unique_timestamps(KW["n_images"], KW["num_cams"])[0])


def test_restatement_is_the_dense_grid_chain():
    """mark / indices_of / world_corners against the reference's own op chain (zeros grid, index_put, nonzero) on random rays that
    leave the box on every side and on end points in (-1, 0) voxels below aabb_min, which the chain marks in voxel 0."""
    g = torch.Generator().manual_seed(5)
    box = torch.tensor([-3.0, -2.0, -1.0, 4.0, 3.0, 2.5])
    res = (9, 7, 5)
    o = torch.rand(600, 3, generator=g) * 8 - 4
    d = torch.nn.functional.normalize(torch.randn(600, 3, generator=g), dim=-1)
    t = torch.rand(600, 1, generator=g) * 4
    vs = V.voxel_size(box, res)
    vc = ((o + d * t - box[:3]) / vs).long()
    keep = ((vc >= 0) & (vc < torch.tensor(res))).all(-1)
    grid = torch.zeros(*res)
    grid[vc[keep, 0], vc[keep, 1], vc[keep, 2]] = 1
    nz = torch.nonzero(grid)
    lin = V.mark(o, d, t, box, res)
    assert torch.equal(V.indices_of(lin, res), nz) and 0 < nz.shape[0] < 600
    assert torch.equal(V.world_corners(lin, box, res), box[:3] + nz * vs)
    below = (((o + d * t - box[:3]) / vs) < 0)[keep].any()
    assert bool(below), "no kept end point lies in the (-1, 0) band: the truncation rule is not exercised"
    far = V.mark(o, d, t, box, res, max_depth=2.0)
    assert set(far.tolist()) <= set(lin.tolist()) and far.numel() < lin.numel()


def test_restatement_reproduces_the_recorded_selection_and_colours():
    z, *_ = load_voxel_case()
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    pca = (t("pca/mat"), t("pca/lo"), t("pca/hi"))
    dens = [t(f"static/density/{k}") for k in range(3)]
    sel = V.mean_selector(dens, 0.5)
    assert torch.equal(sel, torch.stack(dens).mean(0) > 0.5)          # torch's own mean agrees on the recorded values
    kept = V.select_rows(sel, t("static/candidates"))
    assert torch.equal(kept, t("coords")) and 0 < kept.shape[0] < sel.numel()
    np.testing.assert_allclose(V.colours(t("static/feats"), *pca).numpy(), z["colors"], rtol=0, atol=1e-6)
    dsel = V.mean_selector([t("dynamic/0/density")], 0.1)
    dkept = V.select_rows(dsel, t("dynamic/0/candidates"))
    assert int(z["n_dynamic"]) == 1 and torch.equal(dkept, t("dynamic_coords/0")) and 0 < dkept.shape[0] < dsel.numel()
    np.testing.assert_allclose(V.colours(t("dynamic/0/feats"), *pca).numpy(), z["dynamic_colors/0"], rtol=0, atol=1e-6)
    for m, thr in ((torch.stack(dens).mean(0), 0.5), (t("dynamic/0/density"), 0.1)):
        assert float(((m - thr).abs() / thr).min()) > 1e-4


def test_bits_of_and_face_allowance():
    sel = torch.zeros(70, dtype=torch.bool)
    sel[[0, 31, 32, 69]] = True
    assert V.bits_of(sel).tolist() == [1 - 2 ** 31, 1, 32] and V.bits_of(sel).dtype == torch.int32
    # an end point 1 mm from a face is flagged with both voxels at a tolerance of 1 cm, and not at 0.1 mm; the 80 m cut-off counts
    box, res = torch.tensor([0.0, 0.0, 0.0, 8.0, 8.0, 8.0]), (8, 8, 8)
    r = [{"origins": torch.tensor([[0.5, 0.5, 0.5]]), "viewdirs": torch.tensor([[1.0, 0.0, 0.0]]), "d": torch.tensor([2.499])}]
    assert V.face_allowance(r, "d", [torch.tensor([1e-2])], box, res, slack=0.0).tolist() == [2 * 64, 3 * 64]
    assert V.face_allowance(r, "d", [torch.tensor([1e-4])], box, res, slack=0.0).numel() == 0
    assert V.face_allowance(r, "d", [torch.tensor([1e-4])], box, res, max_depth=2.49905, slack=0.0).tolist() == [2 * 64]


@pytest.mark.parametrize("bad", ["shape", "count"])
def test_voxel_grid_rejects_bad_boxes(bad):
    from emernerf_amd._lib import EmerError
    from emernerf_amd.voxels import VoxelGrid, vis_aabb
    with pytest.raises(EmerError):
        if bad == "shape":
            vis_aabb([0.0, 1.0, 2.0])
        else:
            VoxelGrid([0.0, 0.0, 0.0, 4000.0, 4000.0, 4000.0], 1.0, "cpu")      # 6.4e10 voxels
