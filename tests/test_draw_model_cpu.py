"""tests/_draw_model.py is right, and its checkers have power (no GPU): published SplitMix64 vectors, rnd_below's range, the
lidar draw against Python big integers, the race's distribution against torch.multinomial, the ambiguity cap of every race
case tests/test_draw_exact_gpu.py runs, and mutants of every draw kernel, each rejected by the checker the GPU test calls on
the GPU test's own cases.  The radix select of csrc/rays.hip is restated once here, on the fp32-rounded keys, to host the
select mutants."""
import numpy as np
import pytest
import torch

from tests import _draw_model as M

U64 = np.uint64
F32 = np.float32


# ------------------------------------------------------------------------------------------------------ the model
def test_mix64_is_splitmix64():
    """The first four outputs of SplitMix64 from state 0 (the published test vectors): mix64(k G), k = 1 .. 4."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
    assert [int(M.mix64((k * M.G) & M.M64)) for k in (1, 2, 3, 4)] == want
    assert [int(v) for v in M.rnd64(0, np.arange(1, 5, dtype=np.uint64))] == want           # seed 0, counters 1 .. 4
    assert [int(v) for v in M.rnd32(0, np.arange(1, 5, dtype=np.uint64))] == [w >> 32 for w in want]


def test_seed_word_is_read_as_uint64_bits():
    assert int(M.seed_of(-1, 0)) == M.M64 and int(M.seed_of(-0x61C8864680B583EB, 0)) == 0x9E3779B97F4A7C15
    assert int(M.seed_of(1, 0x1111)) == 0x1110
    assert M.next_seed_word(0x7FFFFFFFFFFFFFFF) == -(1 << 63) + 0x9E3779B9 - 1 and M.next_seed_word(-1, 2) == 2 * 0x9E3779B9 - 1


@pytest.mark.parametrize("n", [1, 2, 3, 47, 48, 64, 2 ** 31 - 1])
def test_rnd_below_range(n):
    ctr = np.arange(200_000, dtype=np.uint64)
    for seed in (0, 1, M.M64):
        v = M.rnd_below(seed, ctr, n)
        assert v.min() >= 0 and v.max() < n
        if n <= 64:
            assert v.max() == n - 1 and v.min() == 0
        r = M.rnd32(seed, ctr)
        assert [int(a) for a in v[:64]] == [(int(b) * n) >> 32 for b in r[:64]]


@pytest.mark.parametrize("n_points", [1, 7, 3_000_001, 2 ** 33 + 5, 2 ** 40])
def test_lidar_draw_against_big_integers(n_points):
    for seed_word, salt in M.SEED_SALT:
        got = M.lidar_draw(seed_word, salt, 300, n_points)
        seed = int(M.seed_of(seed_word, salt))
        want = [(int(M.mix64((seed + i * M.G) & M.M64)) * n_points) >> 64 for i in range(300)]
        assert got.tolist() == want and max(want) < n_points


def test_race_samples_the_multinomial_distribution():
    """The device test's statistics (tests/test_kernels_gpu.py) on the model, where draws are cheap: n = 64, k = 8, weights
    rand^3 with two zeros, 20 000 draws over the seed words t 7919 + 1 against 20 000 torch.multinomial draws, five sigma."""
    g = torch.Generator().manual_seed(0)
    n, k, draws = 64, 8, 20_000
    w = torch.rand(n, generator=g) ** 3
    w[5], w[17] = 0.0, 0.0
    w64 = w.numpy().astype(np.float64)
    seeds = (np.arange(draws, dtype=np.uint64) * U64(7919) + U64(1))[:, None]
    r = M.rnd32(seeds, np.arange(n, dtype=np.uint64)[None, :])
    u = ((r >> U64(8)).astype(np.float64) + 1.0) / 16777216.0
    with np.errstate(divide="ignore"):
        keys = np.where(w64 > 0, -np.log(u) / w64, np.inf)
    assert np.array_equal(keys[3], M.race_keys(3 * 7919 + 1, 0, w.numpy()))
    win = np.argpartition(keys, k - 1, axis=1)[:, :k]
    counts = torch.from_numpy(np.bincount(win.reshape(-1), minlength=n)).float()
    assert counts[5] == 0 and counts[17] == 0
    ref = torch.zeros(n)
    gg = torch.Generator().manual_seed(1)
    for _ in range(draws):
        ref[torch.multinomial(w, k, replacement=False, generator=gg)] += 1
    p = ref / draws
    sigma = torch.sqrt(p * (1 - p) / draws).clamp_min(1e-3) * (2 ** 0.5)
    assert float(((counts / draws - p).abs() / sigma).max()) < 5.0


# ------------------------------------------------------------------------------------------------- ambiguity cap
def test_eps_is_the_derived_constant():
    from tests._bounds import E_LOGF
    assert M.EPS == (2 * E_LOGF + 6) * 2.0 ** -24 == 14 * 2.0 ** -24


@pytest.mark.parametrize("name", [c[0] for c in M.RACE_CASES])
def test_ambiguity_cap(name):
    """At most MAY_CAP indices lie within eps of the k-th key, so the set check pins at least k - MAY_CAP winners exactly.  The
    overdraw case is the one whose k-th key is +inf: there `may` is the whole +inf class by definition, `must` is every
    positive weight, and the check pins all of them."""
    c = M.race_case(name)
    print(f"\n[race case] {name}: n = {c['n']}, k = {c['k']}, len(must) = {c['must'].size}, len(may) = {c['may'].size}, kth = {c['kth']:.6g}")
    assert c["k"] <= c["n"] and c["must"].size <= c["k"] - 1 and c["k"] <= c["must"].size + c["may"].size
    if name == "overdraw":
        assert c["kth"] == np.inf and c["must"].size == c["n_pos"] == c["k"] - 5
        assert np.array_equal(c["may"], np.flatnonzero(~(c["w"] > 0)))
    else:
        assert np.isfinite(c["kth"]) and 1 <= c["may"].size <= M.MAY_CAP
        assert c["must"].size >= c["k"] - M.MAY_CAP
    if name.startswith("support"):
        assert c["k"] == c["n_pos"] < c["n"]
    if name.endswith("b"):
        assert np.isnan(c["w"]).sum() == 1 and (c["w"] < 0).sum() == 1


def test_case_list_covers_the_seed_words_and_salts():
    assert {c[4] for c in M.RACE_CASES} == set(M.SEED_WORDS) and {c[5] for c in M.RACE_CASES} == set(M.SALTS)
    assert {c[3] for c in M.RACE_CASES} == {"cubed", "bad", "span"}
    assert any(c[1] > 2048 * 2048 for c in M.RACE_CASES)


# --------------------------------------------------------------------------------- the radix select, restated once
def fp32_key_bits(name):
    """The race keys of a case rounded to fp32, as the order-preserving u32 the device's digits are taken from."""
    c = M.race_case(name)
    with np.errstate(over="ignore"):
        k32 = M.race_keys(c["seed_word"], c["salt"], c["w"]).astype(F32)
    return k32.view(np.uint32) & np.uint32(0x7FFFFFFF)


def radix_select(bits, k, strict=False, keep_need=False, mid_shift=10, late=False):
    """emer_sample_importance's three histogram / select passes and the emit pass (winners in index order; a cursor past its
    share writes nothing).  Mutants: ``strict`` breaks on > instead of >=, ``keep_need`` forgets to subtract acc,
    ``mid_shift`` = 11 takes the middle digit one bit too high, ``late`` tests the count after adding the bin (one bin late)."""
    shifts, bins = (21, mid_shift, 0), (1024, 2048, 1024)
    bits = bits.astype(np.int64)
    prefix, need, pmask = 0, k, 0
    for s, nb in zip(shifts, bins):
        sel = bits[(bits & pmask) == prefix]
        hist = np.bincount((sel >> s) & (nb - 1), minlength=nb)
        acc, b = 0, 0
        while b < nb - 1:
            t = acc + int(hist[b])
            if (t > need) if strict else (t >= need):
                break
            acc, b = t, b + 1
        if late and b < nb - 1:
            acc, b = acc + int(hist[b]), b + 1
        prefix |= b << s
        need = need if keep_need else (need - acc) & 0xFFFFFFFF
        pmask |= (nb - 1) << s
    n_eq, n_lt = need, (k - need) & 0xFFFFFFFF
    out = np.full(k, M.SENT_I64, np.int64)
    lt, eq = np.flatnonzero(bits < prefix), np.flatnonzero(bits == prefix)
    lt = lt[:min(n_lt, k)]
    out[:lt.size] = lt
    room = max(k - min(n_lt, k), 0)
    eq = eq[:min(n_eq, room)]
    out[min(n_lt, k):min(n_lt, k) + eq.size] = eq
    return out


SMALL_RACE = [c[0] for c in M.RACE_CASES if c[1] <= 200_000]


@pytest.mark.parametrize("name", [c[0] for c in M.RACE_CASES])
def test_restated_select_passes_the_checker(name):
    c = M.race_case(name)
    M.check_race(name, radix_select(fp32_key_bits(name), c["k"]))


def _rejected(fn, *a, **kw) -> bool:
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", [dict(keep_need=True), dict(mid_shift=11), dict(late=True)], ids=["acc_not_subtracted", "mid_shift_11", "one_bin_late"])
def test_select_mutants_are_rejected(mutant):
    """A forgotten ``- acc`` is rejected on every case with k > 1.  The middle digit taken one bit too
    high loses bit 10 of the threshold, which shows only where that bit is set in the k-th key; the test one bin late shows
    only where that next bin is occupied: about half of the cases each."""
    cases = [n for n in SMALL_RACE if M.race_case(n)["n"] > 1]
    hit = [n for n in cases if _rejected(M.check_race, n, radix_select(fp32_key_bits(n), M.race_case(n)["k"], **mutant))]
    print(f"\n[power] select {mutant}: rejected on {len(hit)} of {len(cases)} cases: {hit}")
    if "keep_need" in mutant:      # (k = 1 never accumulates: acc stays 0)
        assert hit == [n for n in cases if M.race_case(n)["k"] > 1]
    assert len(hit) >= 3


def test_strict_comparison_in_the_select_is_an_equivalent_mutant():
    """``acc + cum[b] > need`` for ``>=`` does NOT change the set the sampler returns, so no checker of the result can reject
    it.  The two differ only when the running count equals ``need`` exactly at the end of bin b: >= stops there with
    need' = cum[b] (all of the bin), > walks on to the next occupied bin b' (or the last bin) with need' = 0.  Every later
    pass then stops at the first occupied bin with need' = 0, so the final threshold is the smallest key above the k
    winners, n_eq = 0 and n_lt = k: the emit pass writes exactly the keys below it -- the same k indices.  Shown here on
    every case instead of being claimed; tests/test_draw_exact_gpu.py therefore cannot tell the two apart either."""
    differs = 0
    for name in SMALL_RACE:
        k = M.race_case(name)["k"]
        bits = fp32_key_bits(name)
        a, b = radix_select(bits, k), radix_select(bits, k, strict=True)
        assert np.array_equal(np.sort(a), np.sort(b)), name
        M.check_race(name, b)
        differs += not np.array_equal(a, b)
    print(f"\n[power] select > for >=: the same set on all {len(SMALL_RACE)} cases ({differs} with another order of flat_out)")


def test_wrong_race_sets_are_rejected():
    """One winner swapped for the best loser, a repeated index, an index never written, an index out of range."""
    for name in ("n64k8", "n2048k100", "support"):
        c = M.race_case(name)
        good = radix_select(fp32_key_bits(name), c["k"])
        keys = M.race_keys(c["seed_word"], c["salt"], c["w"])
        order = np.argsort(keys)
        swapped = good.copy()
        swapped[np.flatnonzero(good == order[0])[0]] = order[c["k"] + M.MAY_CAP]
        assert _rejected(M.check_race, name, swapped)
        if c["k"] > 1:
            rep = good.copy()
            rep[0] = rep[1]
            assert _rejected(M.check_race, name, rep)
        for bad in (M.SENT_I64, c["n"], -1):
            b = good.copy()
            b[-1] = bad
            assert _rejected(M.check_race, name, b)


# ----------------------------------------------------------------------------------------- mutants of the draws
def _uniform_cases():
    for n in M.UNIFORM_N:
        for H, W in M.UNIFORM_HW:
            for n_cand in M.UNIFORM_NCAND:
                for cand in (None, M.uniform_candidates(n_cand)):
                    for seed_word, salt in M.SEED_SALT:
                        yield seed_word, salt, n, cand, n_cand, H, W


def _mut_uniform(seed, n, cand, n_cand, H, W, swap_xy=False, modulo=False):
    below = (lambda s, c, m: (M.rnd32(s, c) % U64(m)).astype(np.int64)) if modulo else M.rnd_below
    i = np.arange(n, dtype=np.uint64)
    c = below(seed, U64(3) * i, n_cand)
    img = c if cand is None else cand[c]
    cx, cy = (U64(2), U64(1)) if swap_xy else (U64(1), U64(2))
    return img, below(seed, U64(3) * i + cy, H), below(seed, U64(3) * i + cx, W)


def _plus_seed(seed_word, salt):
    return U64(((seed_word & M.M64) + salt) & M.M64)


@pytest.mark.parametrize("mutant", ["xy_counters_swapped", "modulo", "seed_plus_salt"])
def test_uniform_mutants_are_rejected(mutant):
    hit = total = 0
    for seed_word, salt, n, cand, n_cand, H, W in _uniform_cases():
        if mutant == "seed_plus_salt":
            out = _mut_uniform(_plus_seed(seed_word, salt), n, cand, n_cand, H, W)
            matters = salt != 0 and seed_word != 0 and n >= 255 and (H, W) != (1, 1)
        else:
            out = _mut_uniform(M.seed_of(seed_word, salt), n, cand, n_cand, H, W, swap_xy=mutant == "xy_counters_swapped", modulo=mutant == "modulo")
            matters = n >= 255 and (H, W) != (1, 1)
        rej = _rejected(M.check_uniform, *out, seed_word, salt, n, cand, n_cand, H, W, "mutant")
        total += matters
        hit += rej and matters
        assert rej or not matters, f"{mutant} passes at {(seed_word, salt, n, n_cand, H, W)}"
    assert hit == total > 0
    # and the model itself passes its own checker
    for case in list(_uniform_cases())[::97]:
        M.check_uniform(*M.sample_uniform(*case), *case, "model")


def test_lidar_mutants_are_rejected():
    for n, n_points in M.LIDAR_CASES:
        for seed_word, salt in M.SEED_SALT:
            M.check_lidar(M.lidar_draw(seed_word, salt, n, n_points), seed_word, salt, n, n_points, "model")
            if salt != 0 and seed_word != 0 and n_points > 1:
                u = M.rnd64(_plus_seed(seed_word, salt), np.arange(n, dtype=np.uint64))
                assert _rejected(M.check_lidar, M._mulhi64(u, n_points).astype(np.int64), seed_word, salt, n, n_points, "seed + salt")


def _mut_b2p(flat, Hb, Wb, ds, cand, H, W, seed, swap_hw=False, swap_ctr=False):
    i = np.arange(flat.size, dtype=np.uint64)
    if swap_hw:
        Hb, Wb = Wb, Hb
    plane = Hb * Wb
    c = flat // plane
    rem = flat - c * plane
    cy, cx = (U64(1), U64(0)) if swap_ctr else (U64(0), U64(1))
    y = np.clip((rem // Wb) * ds + M.rnd_below(seed, U64(2) * i + cy, ds), 0, H - 1)
    x = np.clip((rem % Wb) * ds + M.rnd_below(seed, U64(2) * i + cx, ds), 0, W - 1)
    return (c if cand is None else cand[c]), y, x


@pytest.mark.parametrize("mutant", ["hb_wb_exchanged", "cell_counters_swapped", "seed_plus_salt"])
def test_buffer_to_pixels_mutants_are_rejected(mutant):
    hit = total = 0
    for Hb, Wb, ds, H, W, n_cand in M.B2P_CASES:
        flat = M.b2p_flat(Hb, Wb, n_cand)
        for cand in (None, M.uniform_candidates(n_cand)):
            for seed_word, salt in M.SEED_SALT:
                args = (flat, Hb, Wb, ds, cand, H, W)
                M.check_buffer_to_pixels(*M.buffer_to_pixels(*args, seed_word, salt), *args, seed_word, salt, "model")
                if mutant == "seed_plus_salt":
                    out, matters = _mut_b2p(*args, _plus_seed(seed_word, salt)), salt != 0 and seed_word != 0 and ds > 1
                else:
                    out = _mut_b2p(*args, M.seed_of(seed_word, salt), swap_hw=mutant == "hb_wb_exchanged", swap_ctr=mutant == "cell_counters_swapped")
                    matters = Hb != Wb if mutant == "hb_wb_exchanged" else ds > 1
                rej = _rejected(M.check_buffer_to_pixels, *out, *args, seed_word, salt, "mutant")
                total += matters
                hit += rej and matters
                assert rej or not matters, f"{mutant} passes at {(Hb, Wb, ds, H, W, seed_word, salt)}"
    assert hit == total > 0
    # the clamp case clamps, the others do not
    for Hb, Wb, ds, H, W, n_cand in M.B2P_CASES:
        assert ((Hb * ds > H) and (Wb * ds > W)) == ((Hb, Wb) == (3, 5))


def test_race_seed_plus_salt_is_rejected():
    """The race cases with a non-zero salt and a non-zero seed word whose result depends on the draw (1 < k < the support), keys drawn
    with seed + salt."""
    names = [c[0] for c in M.RACE_CASES if c[5] != 0 and c[4] != 0 and c[1] <= 200_000 and isinstance(c[2], int) and c[2] > 1]
    assert len(names) >= 2
    for name in names:
        c = M.race_case(name)
        u = ((M.rnd32(_plus_seed(c["seed_word"], c["salt"]), np.arange(c["n"], dtype=np.uint64)) >> U64(8)).astype(np.float64) + 1.0) / 16777216.0
        w = c["w"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            keys = np.where(w > 0, -np.log(u) / w, np.inf)
        assert _rejected(M.check_race, name, np.argsort(keys, kind="stable")[:c["k"]]), name


# ------------------------------------------------------------------------------------------------- error buffer
def test_error_model_follows_the_float64_reference():
    """The fp32 restatement lies inside the float64 bound of tests/_resample_ref.pixel_error_ref."""
    from tests._resample_ref import pixel_error_ref
    for n in M.ERR_CELLS[1:]:
        for with_opa in (False, True):
            pred, gt, opa = M.error_inputs(n, 3, with_opa)
            e, lo, hi = M.pixel_error_rows(pred, gt, opa)
            assert lo == e.min() and hi == e.max() and e.dtype == F32
            v, bound = pixel_error_ref(pred, gt, opa)
            assert (np.abs(M.normalise(e).astype(np.float64) - v) <= bound).all()
            if with_opa:
                assert (opa == F32(0.1)).sum() >= n // 3 and (opa > F32(0.1)).any()


def test_error_mutants_are_rejected():
    for n_imgs in M.ERR_NIMGS:
        maps = np.random.default_rng(n_imgs).random((n_imgs, M.ERR_CELLS_PER_IMG)).astype(F32) + F32(0.25)
        ext = np.stack([maps.min(1), maps.max(1)], 1)
        M.check_normalise(M.normalise(maps, ext), maps, ext, "model")
        lo, hi = ext[:, 0].min(), ext[:, 1].max()
        assert _rejected(M.check_normalise, (maps - lo) / hi, maps, ext, "normalised by hi")
        if n_imgs > 256:   # extrema beyond the first 256 images ignored
            far = maps.copy()
            far[299, 0], far[280, 1] = F32(9.0), F32(0.01)
            ext2 = np.stack([far.min(1), far.max(1)], 1)
            assert _rejected(M.check_normalise, M.normalise(far, ext2[:256]), far, ext2, "first 256 extrema only")
    flat = np.full((3, M.ERR_CELLS_PER_IMG), 0.5, F32)
    assert np.isnan(M.normalise(flat)).all()
    for n in M.ERR_CELLS:
        pred, gt, opa = M.error_inputs(n, 1, True)
        e, lo, hi = M.pixel_error_rows(pred, gt, opa)
        M.check_error_rows(e, [lo, hi], pred, gt, opa, "model")
        e5 = M.pixel_error_rows(pred, gt, np.where(opa == F32(0.1), F32(0.2), opa))[0]      # >= 0.1 instead of > 0.1
        assert _rejected(M.check_error_rows, e5, [e5.min(), e5.max()], pred, gt, opa, ">= 0.1")
        if n > 1024:   # the second trip dropped from the extrema
            big = gt.copy()
            big[n - 1] = pred[n - 1] + F32(40.0)
            e2 = M.pixel_error_rows(pred, big, opa)[0]
            assert _rejected(M.check_error_rows, e2, [e2[:1024].min(), e2[:1024].max()], pred, big, opa, "first trip's extrema only")
