"""The planner of gpsiq_cfilter (csrc/gpsiq_cfilter_plan.h through tests/cfilter_plan.cpp, plain and under
-fsanitize=address,undefined): every plan -- kernel, run, k-steps, runs, grid, LDS bytes -- against the geometry's formulas restated
here, on both sides of both thresholds, at the entry limits of the matrix operand and at every step the int16 path's run shrinks by;
and the operand itself: the host's digit planes, the two byte planes of an int16 stream and the row constants multiplied out in plain
C++ against the direct complex sum."""
import pytest

import _cfilter_plan as cp
import _cfilter_ref as cr

SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
LDS = 65536 - 64


def steps_of(ntaps, decim):
    return -(-(14 * decim + 2 * ntaps) // 64)


def window_bytes(run, decim, steps):
    return 2 * decim * (run - 8) + 64 * steps


def expect(nsamp, in_size, ntaps, decim, phase, kernel):
    """the plan of `kernel` from the geometry's formulas (csrc/gpsiq_filter_geometry.h, gpsiq_cfilter_geometry.h)"""
    nout, nxt = cr.span(nsamp, decim, phase)
    if kernel == cp.GENERIC:
        fit = (8192 - ntaps) // decim + 1
        run, steps = (1024 if fit >= 1024 else fit // 256 * 256), 0
        lds = 4 * ((run - 1) * decim + ntaps) + 4 * ntaps
    else:
        steps = steps_of(ntaps, decim)
        planes = 2 * steps * 1024
        run = next(r for r in (1024, 512, 256) if planes + in_size * window_bytes(r, decim, steps) <= LDS)
        lds = planes + in_size * window_bytes(run, decim, steps)
    runs = -(-nout // run)
    return cp.Plan(kernel, nout, nxt, min(runs, 1 << 20), 256, run, steps, runs, lds)


@SANITIZE
def test_every_plan_is_the_geometrys(sanitize):
    lim = cp.ask([("limits",)], sanitize)[0]
    assert (lim.max_tap, lim.max_run, lim.min_run16, lim.lds, lim.threads) == (32639, 1024, 256, LDS, 256)
    reqs, want = [], []
    for in_size in (1, 2):
        for ntaps in (1, 2, 16, 17, 33, 129, 257, 511, 512):
            for decim in (1, 3, 4, 16):
                for nsamp in (1, 1000, 26_000_000, 2 ** 31 - 1):
                    for force in (cp.FORCE_GENERIC, cp.FORCE_MFMA):
                        phase = decim - 1
                        reqs.append(("plan", nsamp, in_size, ntaps, decim, phase, 100, 100, -100, force))
                        kernel = cp.GENERIC if force == cp.FORCE_GENERIC else (cp.MFMA if in_size == 1 else cp.MFMA16)
                        want.append(expect(nsamp, in_size, ntaps, decim, phase, kernel) if nsamp > phase else cp.Nothing(0, phase - nsamp))
    for r, got, w in zip(reqs, cp.ask(reqs, sanitize), want):
        assert got == w, r


@SANITIZE
def test_both_sides_of_both_thresholds(sanitize):
    lim = cp.ask([("limits",)], sanitize)[0]
    assert (lim.min_taps8, lim.min_taps16) == (5, 17)                # profiles/cfilter_rates.txt
    for in_size, least, matrix in ((1, lim.min_taps8, cp.MFMA), (2, lim.min_taps16, cp.MFMA16)):
        below, above = [1, least - 1], [least, least + 1, 512]
        got = cp.ask([("plan", 5000, in_size, n, d, 0, 10, 10, -10, cp.AUTO) for n in below + above for d in (1, 16)], sanitize)
        assert [p.kernel for p in got] == [cp.GENERIC] * 2 * len(below) + [matrix] * 2 * len(above), (in_size, least)
        # the override wins on either side of the threshold, where the kernel it names can serve
        forced = cp.ask([("plan", 5000, in_size, n, 1, 0, 10, 10, -10, f) for n in (least - 1, least) for f in (cp.FORCE_GENERIC, cp.FORCE_MFMA)], sanitize)
        assert [p.kernel for p in forced] == [cp.GENERIC, matrix] * 2


@SANITIZE
def test_entries_outside_two_signed_bytes_go_to_the_generic_kernel(sanitize):
    cases = [((32639, 32639, -32639), True), ((32640, 0, 0), False), ((0, 32640, 0), False), ((0, 0, -32640), False), ((0, 0, -32768), False),
             ((-32768, 0, 0), True), ((32639, -5, -32639), True)]
    for in_size, matrix in ((1, cp.MFMA), (2, cp.MFMA16)):
        got = cp.ask([("plan", 3000, in_size, 33, 1, 0) + st + (cp.FORCE_MFMA,) for st, _ in cases], sanitize)
        assert [p.kernel for p in got] == [matrix if serves else cp.GENERIC for _, serves in cases]


@SANITIZE
def test_the_int16_run_shrinks_until_planes_and_windows_fit(sanitize):
    """1024, 512 and 256 outputs a run are all taken, each at the first shape that no longer fits the run above it, and the largest
    legal shape still fits 256: inside the contract's ranges the fall to the generic kernel for want of LDS is never taken."""
    seen = {}
    reqs = [("plan", 10 ** 6, 2, ntaps, decim, 0, 1, 1, -1, cp.FORCE_MFMA) for decim in range(1, 17) for ntaps in range(1, 513)]
    for r, p in zip(reqs, cp.ask(reqs, sanitize)):
        ntaps, decim = r[3], r[4]
        assert p == expect(10 ** 6, 2, ntaps, decim, 0, cp.MFMA16), r
        seen.setdefault(p.run, (ntaps, decim))
    assert sorted(seen) == [256, 512, 1024]
    # three of them by hand: 512 taps at decim 1, 8 and 16 (17, 18 and 20 k-steps)
    hand = cp.ask([("plan", 10 ** 6, 2, 512, d, 0, 1, 1, -1, cp.FORCE_MFMA) for d in (1, 8, 16)], sanitize)
    assert [(p.run, p.steps, p.lds) for p in hand] == [(1024, 17, 34816 + 2 * 3120), (512, 18, 36864 + 2 * 9216), (256, 20, 40960 + 2 * 9216)]


@SANITIZE
def test_planes_times_window_is_the_direct_sum(sanitize):
    shapes = [(1, 1), (2, 1), (16, 1), (17, 3), (33, 1), (33, 16), (129, 4), (257, 2), (512, 1), (512, 16), (25, 7)]
    reqs = [("planes", in_size, ntaps, decim, seed, kind) for in_size in (1, 2) for ntaps, decim in shapes for seed in (0, 1, 2) for kind in (0, 1)]
    assert all(cp.ask(reqs, sanitize))
