"""The planner of gpsiq_array_cov / gpsiq_array_combine (csrc/gpsiq_array_plan.h through tests/array_plan.cpp, plain and under
-fsanitize=address,undefined): every plan -- kernel, run, runs, grid, k-steps; lead, slots -- against the geometry's formulas restated
here, on both sides of the threshold and of every edge; and the matrix kernel's layout: the 16 rows of the Gram tile multiplied out in
plain C++ in int32 with the flush every 2047 k-steps, turned into R by the call's own mapping and held to the direct complex sums."""
import pytest

import _array_plan as ap

SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])


def expect_cov(nelem, nsamp, in_size, force, lim):
    if nsamp == 0:
        return None
    can = in_size == 1
    mfma = False if force == ap.FORCE_GENERIC else can if force == ap.FORCE_MFMA else can and nelem >= lim.min_elem
    if mfma:
        steps = -(-nsamp // lim.k)
        run = -(-steps // lim.max_grid)
        run = max(-(-run // 4) * 4, lim.min_run)
        runs = -(-steps // run)
        return ap.CovPlan(ap.MFMA, runs, lim.threads, run, runs, steps)
    runs = -(-nsamp // lim.gen_run)
    return ap.CovPlan(ap.GENERIC, min(runs, lim.gen_grid), lim.threads, lim.gen_run, runs, 0)


@SANITIZE
def test_limits_are_the_contracts(sanitize):
    lim = ap.ask([("limits",)], sanitize)[0]
    assert (lim.max_elem, lim.k, lim.flush, lim.threads) == (8, 64, 2047, 256)
    assert lim.flush * lim.k * 128 * 128 <= 2 ** 31 - 1 < (lim.flush + 1) * lim.k * 128 * 128     # the largest interval that holds
    assert lim.chunk * 2 * 128 * 128 <= 2 ** 31 - 1                  # the generic kernel's int32 partial of one chunk, int8
    assert lim.min_run % 4 == 0 and lim.gen_run % lim.chunk == 0


@SANITIZE
def test_every_covariance_plan_is_the_geometrys(sanitize):
    lim = ap.ask([("limits",)], sanitize)[0]
    run_samples = lim.min_run * lim.k
    sizes = [0, 1, 63, 64, 65, run_samples - 1, run_samples, run_samples + 1, 2 * run_samples, 2 * run_samples + 1, lim.gen_run - 1, lim.gen_run,
             lim.gen_run + 1, lim.gen_run * lim.gen_grid, lim.gen_run * lim.gen_grid + 1, run_samples * lim.max_grid, run_samples * lim.max_grid + 1,
             26_000_000, lim.k * lim.max_grid * 4 * (lim.flush + 1), 2 ** 31 - 1]
    reqs = [("cov", e, n, s, f) for e in (1, 2, 3, 7, 8) for n in sizes for s in (1, 2) for f in (ap.AUTO, ap.FORCE_GENERIC, ap.FORCE_MFMA)]
    for r, got in zip(reqs, ap.ask(reqs, sanitize)):
        assert got == expect_cov(*r[1:], lim), r


@SANITIZE
def test_the_threshold_and_the_override(sanitize):
    lim = ap.ask([("limits",)], sanitize)[0]
    assert lim.min_elem == 2                                         # profiles/array_rates.txt
    auto8 = ap.ask([("cov", e, 100_000, 1, ap.AUTO) for e in range(1, 9)], sanitize)
    assert [p.kernel for p in auto8] == [ap.GENERIC] * (lim.min_elem - 1) + [ap.MFMA] * (9 - lim.min_elem)
    # int16 has no matrix kernel: the override cannot send it there
    got16 = ap.ask([("cov", e, 100_000, 2, f) for e in (1, 8) for f in (ap.AUTO, ap.FORCE_MFMA)], sanitize)
    assert [p.kernel for p in got16] == [ap.GENERIC] * 4
    forced = ap.ask([("cov", e, 100_000, 1, f) for e in (1, 8) for f in (ap.FORCE_GENERIC, ap.FORCE_MFMA)], sanitize)
    assert [p.kernel for p in forced] == [ap.GENERIC, ap.MFMA] * 2


@SANITIZE
def test_a_wave_of_the_largest_plan_flushes(sanitize):
    """The span at which every wave of every workgroup takes flush + 1 k-steps: the size tests/test_gpu_array.py drives the flush with."""
    lim = ap.ask([("limits",)], sanitize)[0]
    nsamp = lim.k * lim.max_grid * 4 * (lim.flush + 1)
    p = ap.ask([("cov", 1, nsamp, 1, ap.FORCE_MFMA)], sanitize)[0]
    assert (p.grid, p.run) == (lim.max_grid, 4 * (lim.flush + 1)) and nsamp == 2 ** 29


@SANITIZE
def test_every_combiner_plan_is_the_geometrys(sanitize):
    lim = ap.ask([("limits",)], sanitize)[0]
    reqs, want = [], []
    for out_size in (1, 2):
        slot = 16 // (2 * out_size)
        for low4 in (0, 4, 8, 12):
            for nsamp in (0, 1, slot - 1, slot, slot + 1, 64 * slot - 1, 64 * slot + 1, 256 * slot, 256 * slot + 1, 26_000_000, 2 ** 31 - 1):
                reqs.append(("combine", nsamp, out_size, low4))
                lead = low4 // (2 * out_size)
                slots = -(-(nsamp + lead) // slot)
                want.append(None if nsamp == 0 else ap.CombinePlan(min(-(-slots // 256), lim.comb_grid), 256, lead, slots))
    for r, got, w in zip(reqs, ap.ask(reqs, sanitize), want):
        assert got == w, r


@SANITIZE
def test_the_gram_tile_is_the_covariance(sanitize):
    """kind 0 random, 1 every byte -128, 2 extremes at random; spans that end inside a k-step; one element to eight"""
    reqs = [("gram", e, n, seed, kind) for e in (1, 2, 3, 7, 8) for n in (1, 63, 64, 65, 1000) for seed in (0, 1) for kind in (0, 1, 2)]
    got = ap.ask(reqs, sanitize)
    assert all(g.flushes == 0 for g in got)
    for r, g in zip(reqs, got):
        if r[4] == 1:                                                # all -128: a sample moves a diagonal entry by 2^14 exactly
            assert g.peak == r[2] * 2 ** 14, r


@SANITIZE
def test_the_flush_bound_is_met_exactly_and_holds(sanitize):
    """One full flush interval plus one k-step, every element all -128: the int32 entries reach 2^31 - 2^20, the last value below the
    wrap that a whole k-step can reach, are flushed once, and the covariance is still the direct sum."""
    lim = ap.ask([("limits",)], sanitize)[0]
    g = ap.ask([("gram", 2, (lim.flush + 1) * lim.k, 5, 1)], sanitize)[0]
    assert g == ap.Gram(2 ** 31 - 2 ** 20, 1)
    g = ap.ask([("gram", 8, (lim.flush + 1) * lim.k - 7, 6, 2)], sanitize)[0]
    assert g.flushes == 1 and g.peak <= 2 ** 31 - 2 ** 20
