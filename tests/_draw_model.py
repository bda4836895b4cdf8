"""The counter-based generator of csrc/rays.hip and the kernels that draw with it, restated in numpy (test helper, not a test
module).  Plain numpy / Python integers: no torch device code, nothing read from any other tree.

Every draw of rays.hip is a pure function of (seed word, salt, index):

    seed        = uint64(seed word) ^ salt                  the seed word is an int64 tensor whose BITS the device reads as uint64
    mix64(z)    = SplitMix64's output function
    rnd32(s, c) = mix64(s + c * G) >> 32,   G = 0x9E3779B97F4A7C15
    rnd_below   = (rnd32 * n) >> 32                         (multiply-shift: no modulo)

so the model below is the SPECIFICATION: the device is held to it bit for bit (tests/test_draw_exact_gpu.py), and
tests/test_draw_model_cpu.py shows that the model is right (published test vectors, big-integer arithmetic, the race's
distribution) and that the checkers below reject wrong kernels.  The GPU file and the CPU file call the same ``check_*``
functions on the same case lists (RACE_CASES, UNIFORM_*, LIDAR_CASES, B2P_CASES, ERR_*), which live here.
"""
import functools

import numpy as np

U64 = np.uint64
F32 = np.float32
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED_STEP = 0x9E3779B9          # what PixelSource._next_seed / LidarSource._next_seed add to the seed word on the device

# ------------------------------------------------------------------------------------------------------- sentinels
SENT_I64 = -0x5A5A5A5A5A5A5A5B  # int64 outputs are handed to the kernels filled with it: an entry the kernel skipped shows
SENT_I32 = 0x5A5A5A5B           # the same for the select workspace (u32 words)
SENT_F32 = 0x7FC5A5A5           # fp32 NaN with a payload no arithmetic produces
GUARD = 16                      # elements in front of and behind every buffer a kernel writes (16 x 4 B keeps 16-byte phase)

# ------------------------------------------------------------------------------------------- seed words and salts
SEED_WORDS = (0, 1, 0x7FFFFFFFFFFFFFFF, -1, -0x61C8864680B583EB)   # the last two: sign bit set, read as the uint64 of the same bits
SALTS = (0, 0xD1B54A32D192ED03)                                      # the second has bit 63 set: it must arrive as a c_uint64
SEED_SALT = tuple((s, t) for s in SEED_WORDS for t in SALTS)


# ------------------------------------------------------------------------------------------------------- generator
def _u64(x):
    """Python int (any sign) or integer array -> uint64 of the same low 64 bits."""
    if isinstance(x, (int, np.integer)):
        return U64(int(x) & M64)
    x = np.asarray(x)
    if x.dtype == np.uint64:
        return x
    return x.astype(np.int64).view(np.uint64)


def mix64(z):
    with np.errstate(over="ignore"):
        z = _u64(z)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def rnd64(seed, ctr):
    with np.errstate(over="ignore"):
        return mix64(_u64(seed) + _u64(ctr) * U64(G))


def rnd32(seed, ctr):
    """uint64 array holding the 32-bit draw."""
    return rnd64(seed, ctr) >> U64(32)


def rnd_below(seed, ctr, n):
    """(rnd32 * n) >> 32 for 1 <= n < 2^32: the product of two 32-bit values fits uint64."""
    assert 1 <= int(n) < (1 << 32)
    return ((rnd32(seed, ctr) * U64(int(n))) >> U64(32)).astype(np.int64)


def seed_of(seed_word: int, salt: int) -> np.uint64:
    """The device's ``seed_word[0] ^ salt``: the int64's bits as uint64, xor the salt."""
    return U64((int(seed_word) & M64) ^ (int(salt) & M64))


def next_seed_word(seed_word: int, advances: int = 1) -> int:
    """The int64 value of the seed word after ``advances`` device-side ``add_(0x9E3779B9)`` (two's complement wraparound)."""
    v = (int(seed_word) + advances * SEED_STEP) & M64
    return v - (1 << 64) if v >> 63 else v


# ------------------------------------------------------------------------------------------------------ the draws
def sample_uniform(seed_word, salt, n, cand, n_cand, H, W):
    """sample_uniform_kernel: counters 3i (candidate), 3i + 1 (x, below W), 3i + 2 (y, below H) -> img, y, x (int64)."""
    seed = seed_of(seed_word, salt)
    i = np.arange(n, dtype=np.uint64)
    c = rnd_below(seed, U64(3) * i, n_cand)
    img = c if cand is None else np.asarray(cand, np.int64)[c]
    x = rnd_below(seed, U64(3) * i + U64(1), W)
    y = rnd_below(seed, U64(3) * i + U64(2), H)
    return img, y, x


def _mulhi64(a, b: int):
    """High 64 bits of a (uint64 array) * b (Python int below 2^64), by 32-bit halves: every partial product and sum fits uint64."""
    m32 = U64(0xFFFFFFFF)
    s32 = U64(32)
    a = _u64(a)
    b0, b1 = U64(b & 0xFFFFFFFF), U64(b >> 32)
    a0, a1 = a & m32, a >> s32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s32) + (p01 & m32) + (p10 & m32)      # < 3 * 2^32
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def lidar_draw(seed_word, salt, n, n_points):
    """lidar_sample_kernel with idx_in == NULL: the high 64 bits of mix64(seed + i G) * n_points (exact for any n_points < 2^63)."""
    assert 1 <= int(n_points) < (1 << 63)
    u = rnd64(seed_of(seed_word, salt), np.arange(n, dtype=np.uint64))
    return _mulhi64(u, int(n_points)).astype(np.int64)


def buffer_to_pixels(flat, Hb, Wb, downscale, cand, H, W, seed_word, salt):
    """buffer_to_pixels_kernel: cell (c, rem / Wb, rem % Wb) of [n_cand][Hb][Wb], times downscale, plus the offsets drawn with
    counters 2i (y) and 2i + 1 (x), clamped into the image -> img, y, x (int64)."""
    seed = seed_of(seed_word, salt)
    flat = np.asarray(flat, np.int64)
    i = np.arange(flat.size, dtype=np.uint64)
    plane = Hb * Wb
    c = flat // plane
    rem = flat - c * plane
    y = (rem // Wb) * downscale + rnd_below(seed, U64(2) * i, downscale)
    x = (rem % Wb) * downscale + rnd_below(seed, U64(2) * i + U64(1), downscale)
    y, x = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
    img = c if cand is None else np.asarray(cand, np.int64)[c]
    return img, y, x


# ------------------------------------------------------------------------------------------------------- the race
# eps: how far the device's fp32 key -logf(u) / w may lie from the model's float64 key, relative.  Built from constants the
# project already owns (tests/_bounds.py), never from the select under test.  With u = 2^-24 the fp32 unit roundoff:
#   * the uniform ((rnd32 >> 8) + 1) / 2^24 is exact in fp32 and in float64, and w is the same fp32 number on both sides;
#   * logf: E_LOGF ulps, at most 2 E_LOGF u relative to its result (the sweep behind E_LOGF includes arguments next to 1);
#   * the fp32 division, taken as rounded no worse than 2.5 ulp: 5 u;
#   * slack: 1 u.
# eps = (2 E_LOGF + 6) 2^-24 = 14 u.  (Two keys are compared, so the window is sound while each key is off by at most
# eps / 2 = 7 u: the measured E_LOGF_MEASURED = 2.143 ulp = 4.3 u plus a correctly rounded division's 1 u is 5.3 u.)
from tests._bounds import E_LOGF  # noqa: E402

EPS = (2.0 * E_LOGF + 6.0) * 2.0 ** -24
MAY_CAP = 2       # len(may) <= MAY_CAP for every committed case (tests/test_draw_model_cpu.py): at least k - 2 winners are pinned


def race_uniforms(seed_word, salt, n, seeds=None):
    """u_i = ((rnd32(seed, i) >> 8) + 1) / 2^24 in (0, 1], float64 (exact)."""
    seed = seed_of(seed_word, salt) if seeds is None else seeds
    r = rnd32(seed, np.arange(n, dtype=np.uint64))
    return ((r >> U64(8)).astype(np.float64) + 1.0) / 16777216.0


def race_keys(seed_word, salt, weights):
    """key_i = -log(u_i) / w_i in float64; +inf where not (w > 0) (zero, negative and NaN weights)."""
    w = np.asarray(weights, F32).astype(np.float64).reshape(-1)
    u = race_uniforms(seed_word, salt, w.size)
    pos = w > 0
    keys = np.full(w.size, np.inf)
    keys[pos] = -np.log(u[pos]) / w[pos]
    return keys


def race_select(keys, k, eps=EPS):
    """(must, may, kth): kth the k-th smallest key, must = {key < kth (1 - eps)}, may = {kth (1 - eps) <= key <= kth (1 + eps)}.
    A correct device result S holds k distinct indices with must <= S <= must | may.  kth = +inf (k exceeds the support):
    must is every finite key, may every +inf key."""
    keys = np.asarray(keys, np.float64)
    assert 1 <= k <= keys.size
    kth = float(np.partition(keys, k - 1)[k - 1])
    lo, hi = kth * (1.0 - eps), kth * (1.0 + eps)
    must = np.flatnonzero(keys < lo)
    may = np.flatnonzero((keys >= lo) & (keys <= hi))
    return must, may, kth


def check_race_set(flat, n, k, must, may, what):
    """flat: the k int64 the device left in flat_out (any order: atomic cursors decide it)."""
    flat = np.asarray(flat, np.int64).reshape(-1)
    assert flat.size == k, f"{what}: {flat.size} entries for k = {k}"
    skipped = int((flat == SENT_I64).sum())
    assert skipped == 0, f"{what}: {skipped} of {k} entries of flat_out were never written"
    assert flat.min() >= 0 and flat.max() < n, f"{what}: index outside [0, {n}): min {flat.min()}, max {flat.max()}"
    s = np.unique(flat)
    assert s.size == k, f"{what}: {k - s.size} repeated indices among {k}"
    missing = np.setdiff1d(must, s)
    assert missing.size == 0, f"{what}: {missing.size} of the {must.size} certain winners are missing (first: {missing[:5].tolist()})"
    extra = np.setdiff1d(s, np.union1d(must, may))
    assert extra.size == 0, f"{what}: {extra.size} entries are neither winners nor within eps of the k-th key (first: {extra[:5].tolist()})"


# (name, n, k, kind, seed word, salt, path).  k: an int, "n" (everything) or "pos" / "pos+5" (the number of positive weights [+ 5]).
# Kinds (race_weights): "cubed" rand^3 with every third entry 0 (indices 2, 5, ...), "bad" the same plus one negative and one NaN
# weight, "span" 10^(-30 rand): spanning 1e-30 .. 1, all positive.
RACE_CASES = (
    ("one", 1, 1, "cubed", 1, 0, "a single weight"),
    ("n64k8", 64, 8, "cubed", 0, 0, "one block, one lane group"),
    ("n64k8b", 64, 8, "bad", -1, SALTS[1], "negative and NaN weights"),
    ("n64k8s", 64, 8, "span", 0x7FFFFFFFFFFFFFFF, 0, "weights over 30 decades"),
    ("n64k1", 64, 1, "cubed", -0x61C8864680B583EB, SALTS[1], "the minimum alone"),
    ("n64k1b", 64, 1, "bad", 0, 0, "the same with a negative and a NaN weight"),
    ("n64k1s", 64, 1, "span", 1, SALTS[1], "the same with weights over 30 decades"),
    ("n2048k100", 2048, 100, "cubed", 1, SALTS[1], "one full block of 8 x 256"),
    ("n2048k100b", 2048, 100, "bad", 0, SALTS[1], "negative and NaN weights"),
    ("n2048k100s", 2048, 100, "span", -1, 0, "weights over 30 decades"),
    ("n2049all", 2049, "n", "span", 0x7FFFFFFFFFFFFFFF, SALTS[1], "second block; k = n = every index, a permutation"),
    ("n200k", 200_000, 1000, "cubed", -0x61C8864680B583EB, 0, "all three digits refine a bucket holding more than `need`"),
    ("n200kb", 200_000, 1000, "bad", 0x7FFFFFFFFFFFFFFF, SALTS[1], "the same with a negative and a NaN weight"),
    ("n200ks", 200_000, 1000, "span", 1, 0, "the same with weights over 30 decades"),
    ("n4300k", 4_300_000, 2048, "cubed", -1, SALTS[1], "n > 2048 x 2048: second grid-stride trip of histogram and emit"),
    ("n4300ks", 4_300_000, 2048, "span", 0, 0, "the same with weights over 30 decades"),
    ("support", 1000, "pos", "cubed", 0, 0, "k = the number of positive weights: the threshold is the largest finite key"),
    ("supportb", 1000, "pos", "bad", 1, SALTS[1], "the same with a negative and a NaN weight outside the support"),
    ("overdraw", 1000, "pos+5", "cubed", -1, 0, "k = positives + 5: the threshold is +inf, five zero-weight indices fill up"),
)


def race_weights(n, kind):
    g = np.random.default_rng(1234 + n)
    r = g.random(n)
    if kind == "span":
        return (10.0 ** (-30.0 * r)).astype(F32)
    w = (r ** 3).astype(F32)
    w[2::3] = 0.0
    if kind == "bad" and n >= 8:
        w[1], w[4] = -0.75, np.nan      # (two entries that were positive)
    return w


@functools.lru_cache(maxsize=None)
def race_case(name):
    """-> dict(n, k, w, seed_word, salt, must, may, kth, n_pos) of a RACE_CASES entry (the model's side, computed once)."""
    _, n, k, kind, seed_word, salt, _ = next(c for c in RACE_CASES if c[0] == name)
    w = race_weights(n, kind)
    n_pos = int((w > 0).sum())
    k = {"n": n, "pos": n_pos, "pos+5": n_pos + 5}.get(k, k)
    must, may, kth = race_select(race_keys(seed_word, salt, w), k)
    return dict(name=name, n=n, k=k, w=w, seed_word=seed_word, salt=salt, must=must, may=may, kth=kth, n_pos=n_pos)


def check_race(name, flat, what=None):
    """The device's flat_out of case ``name`` against the model: the shared checker of the GPU test and the CPU power test."""
    c = race_case(name)
    check_race_set(flat, c["n"], c["k"], c["must"], c["may"], what or f"race {name}")


# --------------------------------------------------------------------------------------------- the other case lists
UNIFORM_N = (1, 255, 257, 5000)
UNIFORM_HW = ((1, 1), (48, 64), (47, 63), (161, 241))
UNIFORM_NCAND = (1, 3, 200)


def uniform_candidates(n_cand):
    """A shuffled candidate list with a repeated entry (n_cand >= 3) over image ids up to 2 n_cand."""
    g = np.random.default_rng(77 + n_cand)
    c = g.permutation(2 * n_cand + 1)[:n_cand].astype(np.int64)
    if n_cand >= 3:
        c[-1] = c[0]
    return c


def check_uniform(img, y, x, seed_word, salt, n, cand, n_cand, H, W, what):
    wi, wy, wx = sample_uniform(seed_word, salt, n, cand, n_cand, H, W)
    for nm, got, want in (("img_idx", img, wi), ("y", y, wy), ("x", x, wx)):
        got = np.asarray(got, np.int64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {nm} differs from the model at {bad.size} of {n} draws (first: i = {bad[0]}, got {got[bad[0]]}, want {want[bad[0]]})"


LIDAR_CASES = ((1, 1), (257, 7), (4096, 10_001), (1000, 3_000_001))   # (n, n_points)


def check_lidar(idx, seed_word, salt, n, n_points, what):
    want = lidar_draw(seed_word, salt, n, n_points)
    assert want.min() >= 0 and want.max() < n_points
    idx = np.asarray(idx, np.int64)
    bad = np.flatnonzero(idx != want)
    assert bad.size == 0, f"{what}: idx differs from the model at {bad.size} of {n} draws (first: i = {bad[0]}, got {idx[bad[0]]}, want {want[bad[0]]})"


# (Hb, Wb, downscale, H, W, n_cand)
B2P_CASES = ((8, 12, 4, 32, 48, 5),      # H = Hb downscale, W = Wb downscale: no clamp
             (3, 5, 16, 40, 70, 4),      # 3 x 16 = 48 > 40 and 5 x 16 = 80 > 70: clamps on both axes
             (1, 1, 1, 1, 1, 3),         # one pixel: every offset is 0
             (9, 13, 4, 37, 53, 6))      # odd sizes, Hb != Wb, an image one pixel larger than the cells cover (H // 4 = 9, W // 4 = 13)
B2P_N = 300


def b2p_flat(Hb, Wb, n_cand, n=B2P_N):
    """Flat cell indices into [n_cand][Hb][Wb]: cell 0 first, the last cell of the last image second, the rest random (repeats allowed)."""
    total = n_cand * Hb * Wb
    f = np.random.default_rng(Hb * 100 + Wb).integers(0, total, n).astype(np.int64)
    f[0], f[1] = 0, total - 1
    return f


def check_buffer_to_pixels(img, y, x, flat, Hb, Wb, downscale, cand, H, W, seed_word, salt, what):
    wi, wy, wx = buffer_to_pixels(flat, Hb, Wb, downscale, cand, H, W, seed_word, salt)
    for nm, got, want in (("img_idx", img, wi), ("y", y, wy), ("x", x, wx)):
        got = np.asarray(got, np.int64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {nm} differs from the model at {bad.size} of {got.size} rays (first: i = {bad[0]}, got {got[bad[0]]}, want {want[bad[0]]})"


# -------------------------------------------------------------------------------------------- error-buffer refresh
ERR_CELLS = (1, 63, 1024, 1025, 2500)   # 1025: the 1024-stride loop's second trip with one lane; 2500: third trip, partial
ERR_NIMGS = (1, 3, 300)                 # 300 > 256: the extrema loop of the normalise kernel takes a second trip
ERR_CELLS_PER_IMG = 7


def pixel_error_rows(pred, gt, opacity=None):
    """pixel_error_image_kernel in fp32, its expression order: ((|d0| + |d1|) + |d2|) / 3, x 5 where the opacity exceeds 0.1f.
    Every operation is rounded once and none can pair into a fused multiply-add -> (row, lo, hi) as the expected bits."""
    pred, gt = np.asarray(pred, F32).reshape(-1, 3), np.asarray(gt, F32).reshape(-1, 3)
    d = np.abs(gt - pred)
    e = ((d[:, 0] + d[:, 1]) + d[:, 2]) / F32(3.0)
    if opacity is not None:
        e = np.where(np.asarray(opacity, F32).reshape(-1) > F32(0.1), e * F32(5.0), e)
    e = e.astype(F32)
    return e, e.min(), e.max()


def normalise(maps, extrema=None):
    """pixel_error_normalise_kernel in fp32: (e - lo) / (hi - lo) with lo / hi the extremes of the per-image (min, max) pairs
    (default: of the maps themselves).  hi == lo gives 0 / 0 = NaN everywhere."""
    maps = np.asarray(maps, F32)
    if extrema is None:
        lo, hi = maps.min(), maps.max()
    else:
        ext = np.asarray(extrema, F32).reshape(-1, 2)
        lo, hi = ext[:, 0].min(), ext[:, 1].max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((maps - F32(lo)) / F32(F32(hi) - F32(lo))).astype(F32)


def error_inputs(n_cells, seed, with_opacity):
    """pred, gt [n_cells, 3] in [0, 1] and opacities of which a third are exactly 0.1f (no x 5), a third above, a third below."""
    g = np.random.default_rng(seed * 7 + n_cells)
    pred, gt = g.random((n_cells, 3)).astype(F32), g.random((n_cells, 3)).astype(F32)
    opa = None
    if with_opacity:
        opa = g.random(n_cells).astype(F32)
        opa[::3] = F32(0.1)
    return pred, gt, opa


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, F32).reshape(-1), np.ascontiguousarray(want, F32).reshape(-1)
    return got.view(np.uint32) == want.view(np.uint32)


def check_error_rows(row, extrema, pred, gt, opacity, what):
    e, lo, hi = pixel_error_rows(pred, gt, opacity)
    ok = _bits_equal(row, e)
    assert ok.all(), (f"{what}: {int((~ok).sum())} of {e.size} cells differ from the fp32 model (first: cell {np.flatnonzero(~ok)[0]}, "
                      f"got {np.asarray(row).reshape(-1)[np.flatnonzero(~ok)[0]]!r}, want {e[np.flatnonzero(~ok)[0]]!r})")
    assert _bits_equal(extrema, [lo, hi]).all(), f"{what}: extrema {np.asarray(extrema).tolist()} != model {[float(lo), float(hi)]}"


def check_normalise(out, maps, extrema, what):
    want = normalise(maps, extrema)
    got = np.asarray(out, F32).reshape(-1)
    ok = _bits_equal(got, want) | (np.isnan(got) & np.isnan(want.reshape(-1)))
    assert ok.all(), (f"{what}: {int((~ok).sum())} of {want.size} cells differ from the fp32 model (first: cell {np.flatnonzero(~ok)[0]}, "
                      f"got {got[np.flatnonzero(~ok)[0]]!r}, want {want.reshape(-1)[np.flatnonzero(~ok)[0]]!r})")
