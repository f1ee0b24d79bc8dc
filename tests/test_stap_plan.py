"""The planner of gpsiq_stap_cov / gpsiq_stap_combine (csrc/gpsiq_stap_plan.h through tests/stap_plan.cpp, plain and under
-fsanitize=address,undefined): every plan -- kernel, row groups, run, runs, grid, k-steps; lead, slots -- against the geometry's
formulas restated here, on both sides of the threshold and of every edge; and the matrix kernel's layout: the tiles on and below the
diagonal multiplied out in plain C++ in int32 with the flush every 2047 k-steps, through an instruction modelled on the measured
register map, sent to the scratch the kernel's way, mirrored and turned into R by the call's own mapping, and held to the direct
complex sums of the shifted rows, heads and tails included."""
import pytest

import _stap_plan as sp

SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
SHAPES = [(1, 1), (1, 8), (2, 4), (4, 2), (8, 1), (3, 3), (4, 5), (5, 5), (8, 4), (4, 8)]


def expect_cov(nelem, ntaps, nsamp, in_size, force, lim):
    if nsamp == 0:
        return None
    rows = nelem * ntaps
    can = in_size == 1
    mfma = False if force == sp.FORCE_GENERIC else can if force == sp.FORCE_MFMA else can and rows >= lim.min_rows
    if mfma:
        steps = -(-nsamp // lim.k)
        run = -(-steps // lim.max_grid)
        run = max(-(-run // 4) * 4, lim.min_run)
        runs = -(-steps // run)
        return sp.CovPlan(sp.MFMA, -(-rows // 8), runs, lim.threads, run, runs, steps)
    runs = -(-nsamp // lim.gen_run)
    return sp.CovPlan(sp.GENERIC, 0, min(runs, lim.gen_grid), lim.threads, lim.gen_run, runs, 0)


@SANITIZE
def test_limits_are_the_contracts(sanitize):
    lim = sp.ask([("limits",)], sanitize)[0]
    assert (lim.max_elem, lim.max_taps, lim.max_rows, lim.k, lim.flush, lim.threads, lim.gram_words) == (8, 8, 32, 64, 2047, 256, 64 * 64)
    assert lim.flush * lim.k * 128 * 128 <= 2 ** 31 - 1 < (lim.flush + 1) * lim.k * 128 * 128     # the largest interval that holds: the array's
    assert lim.chunk * 2 * 128 * 128 <= 2 ** 31 - 1                  # the generic kernel's int32 partial of one chunk, int8
    assert lim.min_run % 4 == 0 and lim.gen_run % lim.chunk == 0
    assert lim.max_rows * lim.max_rows == 4 * lim.threads             # the generic kernel's lanes own four entries at most


@SANITIZE
def test_every_covariance_plan_is_the_geometrys(sanitize):
    lim = sp.ask([("limits",)], sanitize)[0]
    run_samples = lim.min_run * lim.k
    sizes = [0, 1, 63, 64, 65, run_samples - 1, run_samples, run_samples + 1, 2 * run_samples, 2 * run_samples + 1, lim.gen_run - 1, lim.gen_run,
             lim.gen_run + 1, lim.gen_run * lim.gen_grid, lim.gen_run * lim.gen_grid + 1, run_samples * lim.max_grid, run_samples * lim.max_grid + 1,
             26_000_000, lim.k * lim.max_grid * 4 * (lim.flush + 1), 2 ** 31 - 1]
    reqs = [("cov", e, t, n, s, f) for e, t in SHAPES for n in sizes for s in (1, 2) for f in (sp.AUTO, sp.FORCE_GENERIC, sp.FORCE_MFMA)]
    for r, got in zip(reqs, sp.ask(reqs, sanitize)):
        assert got == expect_cov(*r[1:], lim), r


@SANITIZE
def test_the_threshold_the_groups_and_the_override(sanitize):
    lim = sp.ask([("limits",)], sanitize)[0]
    assert lim.min_rows == 2                                         # csrc/gpsiq_stap_plan.h says where it comes from
    shapes = [(e, t) for e in range(1, 9) for t in range(1, 9) if e * t <= 32]
    auto8 = sp.ask([("cov", e, t, 100_000, 1, sp.AUTO) for e, t in shapes], sanitize)
    for (e, t), p in zip(shapes, auto8):
        assert p.kernel == (sp.MFMA if e * t >= lim.min_rows else sp.GENERIC)
        assert p.groups == (-(-e * t // 8) if p.kernel == sp.MFMA else 0)
    assert {p.groups for p in auto8} == {0, 1, 2, 3, 4}
    # int16 has no matrix kernel: the override cannot send it there
    got16 = sp.ask([("cov", e, t, 100_000, 2, f) for e, t in ((1, 1), (8, 4)) for f in (sp.AUTO, sp.FORCE_MFMA)], sanitize)
    assert [p.kernel for p in got16] == [sp.GENERIC] * 4
    forced = sp.ask([("cov", e, t, 100_000, 1, f) for e, t in ((1, 1), (8, 4)) for f in (sp.FORCE_GENERIC, sp.FORCE_MFMA)], sanitize)
    assert [p.kernel for p in forced] == [sp.GENERIC, sp.MFMA] * 2


@SANITIZE
def test_a_wave_of_the_largest_plan_flushes(sanitize):
    """The span at which every wave of every workgroup takes flush + 1 k-steps: the size tests/test_gpu_stap.py drives the flush with."""
    lim = sp.ask([("limits",)], sanitize)[0]
    nsamp = lim.k * lim.max_grid * 4 * (lim.flush + 1)
    p = sp.ask([("cov", 1, 1, nsamp, 1, sp.FORCE_MFMA)], sanitize)[0]
    assert (p.grid, p.run) == (lim.max_grid, 4 * (lim.flush + 1)) and nsamp == 2 ** 28


@SANITIZE
def test_every_combiner_plan_is_the_geometrys(sanitize):
    lim = sp.ask([("limits",)], sanitize)[0]
    reqs, want = [], []
    for out_size in (1, 2):
        slot = 16 // (2 * out_size)
        for low4 in (0, 4, 8, 12):
            for nsamp in (0, 1, slot - 1, slot, slot + 1, 64 * slot - 1, 64 * slot + 1, 256 * slot, 256 * slot + 1, 26_000_000, 2 ** 31 - 1):
                reqs.append(("combine", nsamp, out_size, low4))
                lead = low4 // (2 * out_size)
                slots = -(-(nsamp + lead) // slot)
                want.append(None if nsamp == 0 else sp.CombinePlan(min(-(-slots // 256), lim.comb_grid), 256, lead, slots))
    for r, got, w in zip(reqs, sp.ask(reqs, sanitize), want):
        assert got == w, r


@SANITIZE
def test_the_tiles_are_the_covariance(sanitize):
    """Every shape of the GPU tests: diagonal tiles alone (G = 1), off-diagonal tiles (G = 2 .. 4, the last group ragged for (3, 3),
    (4, 5) and (5, 5)); random data, which no exchange of operands or of the direction of t leaves in place; every byte -128; the
    extremes; spans that end inside a k-step and inside a lane's 16 samples; no head, every head, every other head."""
    reqs = [("gram", e, t, n, seed, kind, heads) for e, t in SHAPES for n, seed in ((1, 0), (t, 1), (63, 2), (65, 3), (200, 4)) for kind in (0, 1, 2)
            for heads in (0, 1, 2)]
    got = sp.ask(reqs, sanitize)
    for r, g in zip(reqs, got):
        groups = -(-r[1] * r[2] // 8)
        assert g.flushes == 0 and g.tiles == groups * (groups + 1) // 2, r
        if r[5] == 1 and r[6] == 1:                                  # all -128 with heads: a sample moves a diagonal entry by 2^14 exactly
            assert g.peak == r[3] * 2 ** 14, r


@SANITIZE
def test_the_flush_bound_is_met_exactly_and_holds(sanitize):
    """One full flush interval plus one k-step, every byte -128, heads too: the int32 entries of every tile, off-diagonal ones
    included, reach 2^31 - 2^20, the last value below the wrap that a whole k-step can reach, are flushed once, and the covariance is
    still the direct sum."""
    lim = sp.ask([("limits",)], sanitize)[0]
    g = sp.ask([("gram", 2, 1, (lim.flush + 1) * lim.k, 5, 1, 0)], sanitize)[0]
    assert g == sp.Gram(2 ** 31 - 2 ** 20, 1, 1)
    g = sp.ask([("gram", 3, 3, (lim.flush + 1) * lim.k, 6, 1, 1)], sanitize)[0]
    assert g == sp.Gram(2 ** 31 - 2 ** 20, 1, 3)
    g = sp.ask([("gram", 2, 4, (lim.flush + 1) * lim.k - 7, 7, 2, 2)], sanitize)[0]
    assert g.flushes == 1 and g.peak <= 2 ** 31 - 2 ** 20
