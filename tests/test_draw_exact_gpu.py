"""The draw kernels of csrc/rays.hip on the device against tests/_draw_model.py, the numpy restatement of the counter-based
generator (whose own correctness and power tests/test_draw_model_cpu.py shows without a GPU):

* emer_sample_uniform, emer_buffer_to_pixels and the draw of emer_lidar_sample_rays (idx_in == NULL): bit for bit;
* emer_sample_importance: as a set -- k distinct indices S with must <= S <= must | may, where ``may`` holds the at most two
  indices whose float64 key lies within eps of the k-th (the order of flat_out is decided by atomic cursors and is not pinned);
* emer_pixel_error_image / emer_pixel_error_normalise: bit for bit against the fp32 restatement;
* PixelSource.get_train_rays and LidarSource.sample_uniform_rays / get_train_rays: the salts, the split of a batch into its
  uniform and buffer parts, and the seed word's advance of 0x9E3779B9 per batch.

Every buffer a kernel writes sits between guards of ``M.GUARD`` sentinels that must come back intact, and pure outputs are
handed over filled with the sentinel, so an entry a kernel skipped shows.  Shapes are the smallest that reach the path they
name; the case lists live in tests/_draw_model.py, where the CPU file guards them too.
"""
import numpy as np
import pytest
import torch

from tests import _draw_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
_NP = {torch.int64: (np.int64, M.SENT_I64), torch.int32: (np.uint32, M.SENT_I32), torch.float32: (np.uint32, M.SENT_F32)}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Guarded:
    """A device buffer [GUARD sentinels | n elements | GUARD sentinels] of int64, int32 or float32 (NaN sentinel, compared by
    its bits).  data = None hands the kernel a pure output: sentinels throughout."""

    def __init__(self, n, dtype, data=None):
        self.n, self.dtype = n, dtype
        np_t, self.sent = _NP[dtype]
        host = np.full(M.GUARD + n + M.GUARD, self.sent, np_t)
        if data is not None:
            d = np.ascontiguousarray(data).reshape(-1)
            host[M.GUARD:M.GUARD + n] = d.view(np.uint32) if dtype == torch.float32 else d
        as_torch = (lambda a: torch.from_numpy(a.view(np.int32) if np_t is np.uint32 else a))   # noqa: E731
        self._sentinels = as_torch(np.full(host.size, self.sent, np_t))
        self.buf = as_torch(host).to(_dev())
        self.view = self.buf[M.GUARD:M.GUARD + n]
        if dtype == torch.float32:
            self.view = self.view.view(torch.float32)

    def refill(self):
        self.buf.copy_(self._sentinels)

    def result(self, what):
        host = self.buf.cpu().numpy()
        raw = host.view(np.uint32) if self.dtype != torch.int64 else host
        assert (raw[:M.GUARD] == self.sent).all() and (raw[M.GUARD + self.n:] == self.sent).all(), f"{what}: a guard was overwritten"
        body = host[M.GUARD:M.GUARD + self.n]
        return body.view(F32).copy() if self.dtype == torch.float32 else body.copy()


def _call(name, *args):
    from emernerf_amd import _lib
    _lib.call(name, *args)


def _ptr(t):
    from emernerf_amd import ops
    return ops._ptr(t.view if isinstance(t, Guarded) else t)


def _stream():
    import ctypes
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(_dev())


def _seed(seed_word):
    return torch.tensor([seed_word], dtype=torch.int64, device=_dev())


# --------------------------------------------------------------------------------------------------- sample_uniform
@pytest.mark.parametrize("H,W", M.UNIFORM_HW)
def test_sample_uniform_is_the_model(hip_lib, H, W):
    """img / y / x bit for bit: n = 1, one block short by one, one block plus one, 20 blocks; 1, 3 and 200 candidates, as a
    shuffled list with a repeated entry and as NULL; every seed word with both salts."""
    for n in M.UNIFORM_N:
        for n_cand in M.UNIFORM_NCAND:
            for cand in (None, M.uniform_candidates(n_cand)):
                dc = _t(cand)
                for seed_word, salt in M.SEED_SALT:
                    what = f"sample_uniform n={n} H={H} W={W} n_cand={n_cand} cand={'list' if cand is not None else 'NULL'} seed={seed_word:#x} salt={salt:#x}"
                    sw = _seed(seed_word)
                    img, y, x = (Guarded(n, torch.int64) for _ in range(3))
                    _call("emer_sample_uniform", _ptr(sw), salt, n, _ptr(dc), n_cand, H, W, _ptr(img), _ptr(y), _ptr(x), _stream())
                    M.check_uniform(img.result(what), y.result(what), x.result(what), seed_word, salt, n, cand, n_cand, H, W, what)
                    assert int(sw.cpu()) == seed_word, f"{what}: the kernel wrote the seed word"


# ------------------------------------------------------------------------------------------------------- lidar draw
@pytest.mark.parametrize("n,n_points", M.LIDAR_CASES)
def test_lidar_draw_is_the_model(hip_lib, n, n_points):
    """idx_out bit for bit and the four gathers exactly origins / dirs / ranges / ts [idx], with and without timestamps, with
    and without idx_out.  n_points >= 2^32 cannot be reached on the device: the kernel always gathers, so the four source
    arrays would need more than 2^32 rows; tests/test_draw_model_cpu.py holds the 64-bit product's arithmetic to Python
    integers up to 2^40 instead."""
    g = torch.Generator().manual_seed(n_points)
    src = [torch.rand(n_points, c, generator=g).to(_dev()) for c in (3, 3, 1, 1)]
    for with_ts in (True, False):
        for with_idx in (True, False):
            for seed_word, salt in M.SEED_SALT:
                what = f"lidar n={n} n_points={n_points} ts={with_ts} idx_out={with_idx} seed={seed_word:#x} salt={salt:#x}"
                sw = _seed(seed_word)
                idx = Guarded(n, torch.int64) if with_idx else None
                o, d, r = Guarded(3 * n, torch.float32), Guarded(3 * n, torch.float32), Guarded(n, torch.float32)
                t = Guarded(n, torch.float32) if with_ts else None
                _call("emer_lidar_sample_rays", _ptr(sw), salt, n, n_points, None, _ptr(src[0]), _ptr(src[1]), _ptr(src[2]),
                      _ptr(src[3]) if with_ts else None, _ptr(idx) if with_idx else None, _ptr(o), _ptr(d), _ptr(r), _ptr(t) if with_ts else None, _stream())
                want = M.lidar_draw(seed_word, salt, n, n_points)
                if with_idx:
                    M.check_lidar(idx.result(what), seed_word, salt, n, n_points, what)
                wi = _t(want)
                for nm, buf, s in (("origins", o, src[0]), ("dirs", d, src[1]), ("ranges", r, src[2])) + ((("ts", t, src[3]),) if with_ts else ()):
                    got = buf.result(f"{what} {nm}")
                    assert np.array_equal(got.view(np.uint32), s[wi].cpu().numpy().reshape(-1).view(np.uint32)), f"{what}: {nm} != source[idx]"


# ------------------------------------------------------------------------------------------------- importance race
@pytest.fixture(scope="module")
def workspace():
    """ONE select workspace for every race call of the module, never cleared between calls: race_init_kernel has to reset the
    state and the histogram whatever the call before left there (the first call finds sentinels)."""
    return Guarded(4 + 2048, torch.int32)


@pytest.mark.parametrize("name", [c[0] for c in M.RACE_CASES])
def test_sample_importance_is_the_models_set(hip_lib, workspace, name):
    """sorted(flat_out) holds k distinct indices, every index whose key lies below (1 - eps) x the k-th key, and nothing beyond
    (1 + eps) x it (tests/test_draw_model_cpu.py: at most 2 indices are that close, so at least k - 2 winners are pinned).  Two
    consecutive calls on the same workspace.  The case "overdraw" asks for 5 more than carry weight: every positive index,
    five distinct others, nothing past flat_out[k - 1]."""
    c = M.race_case(name)
    n, k = c["n"], c["k"]
    w, sw = _t(c["w"]), _seed(c["seed_word"])
    out = Guarded(k, torch.int64)
    for call in (1, 2):
        what = f"race {name} (n={n}, k={k}) call {call}"
        _call("emer_sample_importance", _ptr(w), n, _ptr(sw), c["salt"], k, _ptr(workspace), _ptr(out), _stream())
        flat = out.result(what)
        workspace.result(what)
        M.check_race(name, flat, what)
        if name == "overdraw":
            pos = c["w"][flat] > 0
            assert int(pos.sum()) == c["n_pos"] and int((~pos).sum()) == 5
        out.refill()
    print(f"\n[race] {name}: n = {n}, k = {k}, len(must) = {c['must'].size}, len(may) = {c['may'].size}")


# ------------------------------------------------------------------------------------------------ buffer_to_pixels
@pytest.mark.parametrize("Hb,Wb,ds,H,W,n_cand", M.B2P_CASES)
def test_buffer_to_pixels_is_the_model(hip_lib, Hb, Wb, ds, H, W, n_cand):
    flat = M.b2p_flat(Hb, Wb, n_cand)
    assert flat[0] == 0 and flat[1] == n_cand * Hb * Wb - 1
    df = _t(flat)
    for cand in (None, M.uniform_candidates(n_cand)):
        dc = _t(cand)
        for seed_word, salt in M.SEED_SALT:
            what = f"buffer_to_pixels {(Hb, Wb, ds, H, W)} cand={'list' if cand is not None else 'NULL'} seed={seed_word:#x} salt={salt:#x}"
            sw = _seed(seed_word)
            img, y, x = (Guarded(flat.size, torch.int64) for _ in range(3))
            _call("emer_buffer_to_pixels", _ptr(df), flat.size, Hb, Wb, ds, _ptr(dc), H, W, _ptr(sw), salt, _ptr(img), _ptr(y), _ptr(x), _stream())
            M.check_buffer_to_pixels(img.result(what), y.result(what), x.result(what), flat, Hb, Wb, ds, cand, H, W, seed_word, salt, what)


# ---------------------------------------------------------------------------------------------- through the classes
def _refreshed_pixel_source():
    from emernerf_amd.pixel_source import PixelSource
    dev = _dev()
    src = PixelSource.synthetic(dev, num_imgs=6, height=32, width=48, buffer_ratio=0.2)
    src.build_pixel_error_buffer()
    Hb, Wb = src.pixel_error_maps.shape[1:]
    g = torch.Generator().manual_seed(11)
    for i in range(src.num_imgs):
        src.accumulate_pixel_error(i, torch.rand(Hb, Wb, 3, generator=g).to(dev), torch.rand(Hb, Wb, 3, generator=g).to(dev))
    src.finish_pixel_error_maps()
    return src


@pytest.mark.parametrize("cand", [None, [4, 1, 5]], ids=["all_images", "candidates"])
def test_pixel_source_batches_are_the_model(hip_lib, cand):
    """get_train_rays(400) with buffer_ratio 0.2 after a refresh of the error buffer: the first 400 - int(400 x 0.2) = 320 rays
    are the uniform draw with _SALT_UNIFORM, the last 80 the race over the (candidates') error maps with _SALT_RACE, each
    moved inside its cell by the offsets drawn with _SALT_CELL for its position among the 80; ONE advance of the seed word
    by 0x9E3779B9 per batch (int64 wraparound included), two batches per seed word."""
    from emernerf_amd import pixel_source as PS
    src = _refreshed_pixel_source()
    H, W, ds = src.HEIGHT, src.WIDTH, src.buffer_downscale
    maps = src.pixel_error_maps.cpu().numpy()
    Hb, Wb = maps.shape[1:]
    assert (Hb, Wb, ds) == (8, 12, 4) and maps.min() == 0.0 and maps.max() == 1.0
    wts = maps if cand is None else maps[cand]
    n_c = src.num_imgs if cand is None else len(cand)
    npc = None if cand is None else np.asarray(cand, np.int64)
    n, n_roi = 400, 80
    for seed_word in M.SEED_WORDS:
        src.seed_word.fill_(seed_word)
        for batch_no in range(2):
            s0 = int(src.seed_word.cpu())
            assert s0 == M.next_seed_word(seed_word, batch_no)
            what = f"get_train_rays seed={seed_word:#x} batch {batch_no}"
            b = src.get_train_rays(n, cand)
            assert int(src.seed_word.cpu()) == M.next_seed_word(s0), f"{what}: the seed word advances by 0x9E3779B9 once per batch"
            img, pc = b["img_idx"].cpu().numpy(), b["pixel_coords"].cpu().numpy()
            assert img.shape == (n,) and pc.shape == (n, 2)
            y, x = np.rint(pc[:, 0] * H).astype(np.int64), np.rint(pc[:, 1] * W).astype(np.int64)
            assert np.array_equal(pc[:, 0], y.astype(F32) / F32(H)) and np.array_equal(pc[:, 1], x.astype(F32) / F32(W))
            M.check_uniform(img[:n - n_roi], y[:n - n_roi], x[:n - n_roi], s0, PS._SALT_UNIFORM, n - n_roi, npc, n_c, H, W, f"{what} uniform part")
            bi, by, bx = img[n - n_roi:], y[n - n_roi:], x[n - n_roi:]
            c = bi if cand is None else np.array([cand.index(int(v)) if int(v) in cand else -1 for v in bi], np.int64)
            assert c.min() >= 0 and c.max() < n_c, f"{what}: a buffer ray outside the candidate images"
            flat = (c * Hb + by // ds) * Wb + bx // ds
            must, may, _ = M.race_select(M.race_keys(s0, PS._SALT_RACE, wts.reshape(-1)), n_roi)
            assert may.size <= M.MAY_CAP
            M.check_race_set(flat, wts.size, n_roi, must, may, f"{what} buffer part")
            M.check_buffer_to_pixels(bi, by, bx, flat, Hb, Wb, ds, npc, H, W, s0, PS._SALT_CELL, f"{what} sub-cell offsets")


def test_lidar_source_draws_are_the_model(hip_lib):
    """sample_uniform_rays over all points and over the cached scans of a candidate list, and get_train_rays' gather of a
    fresh draw: _SALT_LIDAR, one advance per call."""
    from emernerf_amd import lidar_source as LS
    src = LS.LidarSource.synthetic(_dev(), num_timesteps=5, points_per_scan=64)
    for seed_word in M.SEED_WORDS:
        src.seed_word.fill_(seed_word)
        idx = src.sample_uniform_rays(300).cpu().numpy()
        M.check_lidar(idx, seed_word, LS._SALT_LIDAR, 300, 320, f"LidarSource all points seed={seed_word:#x}")
        s1 = int(src.seed_word.cpu())
        assert s1 == M.next_seed_word(seed_word)
        idx = src.sample_uniform_rays(257, [1, 3]).cpu().numpy()
        M.check_lidar(idx, s1, LS._SALT_LIDAR, 257, 128, f"LidarSource cached scans seed={seed_word:#x}")
        s2 = int(src.seed_word.cpu())
        assert s2 == M.next_seed_word(seed_word, 2)
        rays = src.get_train_rays(200, [1, 3])
        assert int(src.seed_word.cpu()) == M.next_seed_word(seed_word, 3)
        wi = _t(M.lidar_draw(s2, LS._SALT_LIDAR, 200, 128))
        for key, cached in (("lidar_origins", src.cached_origins), ("lidar_viewdirs", src.cached_directions), ("lidar_ranges", src.cached_ranges),
                            ("lidar_normed_timestamps", src.cached_normalized_timestamps)):
            assert torch.equal(rays[key], cached[wi]), f"LidarSource.get_train_rays {key} seed={seed_word:#x}"


# ------------------------------------------------------------------------------------------- error-buffer refresh
@pytest.mark.parametrize("with_opacity", [False, True], ids=["no_opacity", "opacity"])
@pytest.mark.parametrize("n_cells", M.ERR_CELLS)
def test_pixel_error_image_is_the_fp32_model(hip_lib, n_cells, with_opacity):
    """The row and its (min, max) bit for bit: one cell (1023 lanes without one), 63, exactly 1024, 1025 (the stride loop's
    second trip with one lane), 2500; a third of the opacities are exactly 0.1f and do not take the x 5."""
    pred, gt, opa = M.error_inputs(n_cells, 1, with_opacity)
    what = f"pixel_error_image n_cells={n_cells} opacity={with_opacity}"
    row, ext = Guarded(n_cells, torch.float32), Guarded(2, torch.float32)
    dp, dg, do = _t(pred), _t(gt), _t(opa)
    _call("emer_pixel_error_image", _ptr(dp), _ptr(dg), _ptr(do) if with_opacity else None, n_cells, _ptr(row), _ptr(ext), _stream())
    M.check_error_rows(row.result(what), ext.result(what), pred, gt, opa, what)


@pytest.mark.parametrize("n_imgs", M.ERR_NIMGS)
def test_pixel_error_normalise_is_the_fp32_model(hip_lib, n_imgs):
    """7 cells per image, in place, bit for bit.  With 300 images the global extremes sit in images 280 and 299: the extrema
    loop's second trip.  Then the two kernels chained as PixelSource chains them, and the all-equal buffer: NaN everywhere."""
    cells = M.ERR_CELLS_PER_IMG
    maps = np.random.default_rng(n_imgs).random((n_imgs, cells)).astype(F32) + F32(0.25)
    if n_imgs > 256:
        maps[299, 0], maps[280, 1] = F32(9.0), F32(0.01)
    ext = np.stack([maps.min(1), maps.max(1)], 1)
    what = f"pixel_error_normalise n_imgs={n_imgs}"
    buf, de = Guarded(maps.size, torch.float32, maps), _t(ext)
    _call("emer_pixel_error_normalise", _ptr(buf), maps.size, _ptr(de), n_imgs, _stream())
    M.check_normalise(buf.result(what), maps, ext, what)
    # the image kernel's rows and extrema feeding the normalisation
    buf, dext = Guarded(maps.size, torch.float32), Guarded(2 * n_imgs, torch.float32)
    rows = []
    for i in range(n_imgs):
        pred, gt, opa = M.error_inputs(cells, 100 + i, i % 2 == 0)
        rows.append(M.pixel_error_rows(pred, gt, opa)[0])
        dp, dg, do = _t(pred), _t(gt), _t(opa)
        _call("emer_pixel_error_image", _ptr(dp), _ptr(dg), _ptr(do) if opa is not None else None, cells,
              _ptr(buf.view[i * cells:]), _ptr(dext.view[2 * i:]), _stream())
        torch.cuda.current_stream().synchronize()   # the inputs stay alive until the kernel has read them
    rows = np.stack(rows)
    got_ext = dext.result(f"{what} chained extrema")
    assert np.array_equal(got_ext.view(np.uint32), np.stack([rows.min(1), rows.max(1)], 1).reshape(-1).view(np.uint32))
    _call("emer_pixel_error_normalise", _ptr(buf), maps.size, _ptr(dext), n_imgs, _stream())
    M.check_normalise(buf.result(f"{what} chained"), rows, got_ext, f"{what} chained")
    # every cell equal: 0 / 0
    flat = np.full((n_imgs, cells), 0.5, F32)
    buf, de = Guarded(flat.size, torch.float32, flat), _t(np.tile(np.array([0.5, 0.5], F32), n_imgs))
    _call("emer_pixel_error_normalise", _ptr(buf), flat.size, _ptr(de), n_imgs, _stream())
    assert np.isnan(buf.result(f"{what} all equal")).all()
