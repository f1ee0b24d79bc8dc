"""The resampler stage on the CPU: tests/_resample_ref.py (the numpy restatement the GPU tests compare every byte with) against a
second, scalar statement of the contract of include/gpsiq_rows.h ("Resample"), the identity table, continuation in pieces, the
library's gpsiq_resample_span, gpsiq_resample_step and gpsiq_resample_design, the planner of the calls (tests/resample_plan.cpp, also
under ASan + UBSan), the refusals that need no device and the argument checks of gpsiq_runahead --resample."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _resample_plan as rp
import _resample_ref as rr
import gpsiq
from gpsiq.abi import SC08, SC16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 32
STEPS = [ONE, ONE + 1, ONE - 1, 1 << 29, 1 << 35, 3 << 31, round(ONE * 2.6 / 2.048), round(ONE * (1 + 20e-6)), 0x16A09E667]


# ---- the two statements of the contract -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_size", [SC08, SC16])
@pytest.mark.parametrize("out_size", [SC08, SC16])
def test_numpy_and_scalar_statements_agree(in_size, out_size):
    rng = np.random.default_rng(100 * in_size + out_size)
    clipped_somewhere = False
    cases = [(0, 1, 9, 0, 0, ONE, 0), (0, 3, 20, 5, 1, ONE + 12345, ONE - 1), (1, 2, 17, 3, 1, 3 << 31, 1 << 31), (3, 7, 40, 16, 1, 1 << 29, 0),
             (5, 16, 33, 8, 0, 1 << 35, 7), (8, 4, 50, 14, 1, STEPS[6], ONE - 1), (2, 5, 1, 0, 1, 1 << 30, 99), (4, 9, 3, 16, 0, STEPS[8], 5 * ONE),
             (6, 12, 60, 6, 1, STEPS[7], (1 << 32) - (1 << 20))]
    for L, ntaps, nsamp, shift, interp, step, pos0 in cases:
        x = rr.full_range(rng, nsamp, in_size)
        head = rr.full_range(rng, ntaps - 1, in_size)
        taps = rr.random_table(rng, L, ntaps, 65535 if ntaps > 2 else None)
        for h in (None, head):
            a = rr.resample_ref(x, h, taps, L, shift, interp, step, pos0, out_size)
            b = rr.resample_scalar(x, h, taps, L, shift, interp, step, pos0, out_size)
            assert a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and a[1:] == b[1:], (L, ntaps, nsamp, step, pos0)
            assert len(a[0]) == rr.span(nsamp, pos0, step)[0]
            clipped_somewhere |= a[1] > 0
            # any range of j on its own
            lo, hi = len(a[0]) // 3, len(a[0]) - len(a[0]) // 4
            part = rr.resample_ref(x, h, taps, L, shift, interp, step, pos0, out_size, lo, hi)
            assert np.array_equal(part[0], a[0][lo:hi]) and part[2:] == a[2:]
    assert clipped_somewhere


def test_phase_weight_rounding_and_clamp_by_hand():
    # two phases, one tap: rows 10, 20 and the row "one sample later" 30; x = 8 everywhere.  pos 0: q 0, mu 0 -> 80.  pos 0.25: q 0,
    # mu 128 -> (128 * 80 + 128 * 160 + 128) >> 8 = 120.  pos 0.5: q 1, mu 0 -> 160.  pos 0.75: q 1, mu 128 -> (160 + 240) / 2 = 200.
    taps = [[10], [20], [30]]
    x = np.full((4, 2), 8, np.int16)
    out, c, nout, nxt = rr.resample_ref(x, None, taps, 1, 0, 1, ONE // 4, 0, SC16)
    assert out[:4, 0].tolist() == [80, 120, 160, 200] and c == 0 and nout == 16 and nxt == 0
    out, *_ = rr.resample_ref(x, None, taps, 1, 0, 0, ONE // 4, 0, SC16)
    assert out[:4, 0].tolist() == [80, 80, 160, 160]
    # without interp the filter's rounding: floor((a0 + 1) / 2): -3 -> -1, 3 -> 2, -1 -> 0
    out, c, *_ = rr.resample_ref([[-3, 3], [-1, 1]], None, [[1], [1]], 0, 1, 0, ONE, 0, SC08)
    assert out.tolist() == [[-1, 2], [0, 1]] and c == 0
    # the clamp is symmetric and counted
    out, c, *_ = rr.resample_ref(np.array([[-128, 100], [63, -64]], np.int8), None, [[2], [2]], 0, 0, 0, ONE, 0, SC08)
    assert out.tolist() == [[-127, 127], [126, -127]] and c == 3
    # causal, with a head: y(0) = 3 x(0) + 5 x(-1)
    out, *_ = rr.resample_ref([[10, -10]], [[1, 2]], [[3, 5], [0, 0]], 0, 0, 0, ONE, 0, SC16)
    assert out.tolist() == [[35, -20]]


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("delay", [0, 3, 6])
def test_identity_table_gives_the_input_delayed(interp, delay):
    """step 2^32, pos0 0, one phase, a single tap of 2^shift: expected is the input itself, not a second evaluation of the contract"""
    rng = np.random.default_rng(delay)
    shift, ntaps = 9, 7
    x = rr.full_range(rng, 200, SC16)
    x[x == -32768] = -32767                                          # (the symmetric clamp would change the most negative value)
    row = np.zeros(ntaps, np.int16)
    row[delay] = 1 << shift
    nxt_row = np.zeros(ntaps, np.int16)                              # "phase 0, one sample later": the same tap a place earlier
    if delay:
        nxt_row[delay - 1] = 1 << shift
    out, c, nout, nxt = rr.resample_ref(x, None, [row, nxt_row], 0, shift, interp, ONE, 0, SC16)
    want = np.concatenate([np.zeros((delay, 2), np.int16), x[:len(x) - delay]])
    assert nout == 200 and nxt == 0 and c == 0 and np.array_equal(out, want)


@pytest.mark.parametrize("step", STEPS)
def test_pieces_equal_the_whole(step):
    rng = np.random.default_rng(step % 1000)
    L, ntaps, nsamp, shift = 4, 9, 131, 4
    x = rr.full_range(rng, nsamp, SC16)
    taps = rr.random_table(rng, L, ntaps)
    for interp, pos0 in ((0, 0), (1, ONE - 1), (1, 1 << 31)):
        whole, cw, nw, nxw = rr.resample_ref(x, None, taps, L, shift, interp, step, pos0, SC08)
        for cut in (1, ntaps - 2, ntaps - 1, nsamp // 2):
            hist = np.zeros((ntaps - 1, 2), np.int16)
            parts, clipped, pos, empty = [], 0, pos0, 0
            for piece in (x[:cut], x[cut:cut + 5], x[cut + 5:cut + 6], x[cut + 6:]):      # pieces shorter than the history, one of a single sample
                o, c, n, nxt = rr.resample_ref(piece, hist, taps, L, shift, interp, step, pos, SC08)
                assert (n, nxt) == rr.span(len(piece), pos, step) and len(o) == n
                empty += n == 0
                parts.append(o)
                clipped += c
                pos = nxt
                hist = np.concatenate([hist, piece])[len(piece):]
            assert np.array_equal(np.concatenate(parts), whole) and clipped == cw and pos == nxw and sum(len(p) for p in parts) == nw, (interp, cut)
            if step >= 1 << 33:
                assert empty > 0                                     # a piece of one sample between outputs two or more apart


# ---- the library's host arithmetic ------------------------------------------------------------------------------------------------

def brute_span(nsamp, pos0, step):
    j = 0
    while (pos0 + j * step) >> 32 < nsamp:
        j += 1
    return j, pos0 + j * step - nsamp * ONE


def test_resample_span_is_the_formulas():
    reqs = []
    for nsamp in (0, 1, 2, 15, 16, 17, 1000):
        for step in STEPS:
            for pos0 in (0, 1, ONE - 1, 1 << 31, nsamp * ONE - 1 if nsamp else 0, nsamp * ONE, nsamp * ONE + 12345, (1 << 63) - 1):
                want = brute_span(nsamp, pos0, step) if pos0 < nsamp * ONE else (0, pos0 - nsamp * ONE)
                assert rr.span(nsamp, pos0, step) == want
                assert gpsiq.resample_span(nsamp, pos0, step) == want, (nsamp, pos0, step)
                reqs.append((("span", nsamp, pos0, step), want))
    # spans no loop can walk: the defining property instead.  nsamp * 2^32 needs more than 64 bits from 2^32 samples on
    for nsamp in (2 ** 31 - 1, 2 ** 32, 2 ** 40, 2 ** 60 - 1):
        for step in (1 << 29, ONE - 1, 1 << 35, 0x16A09E667):
            for pos0 in (0, ONE - 1, (1 << 63) - 1):
                nout, nxt = gpsiq.resample_span(nsamp, pos0, step)
                assert (nout, nxt) == rr.span(nsamp, pos0, step)
                if pos0 < nsamp * ONE:
                    assert (pos0 + (nout - 1) * step) >> 32 < nsamp <= (pos0 + nout * step) >> 32 and 0 <= nxt < step
                else:
                    assert nout == 0 and nxt == pos0 - nsamp * ONE
                reqs.append((("span", nsamp, pos0, step), (nout, nxt)))
    for sanitize in (False, True):
        for (r, want), got in zip(reqs, rp.ask([r for r, _ in reqs], sanitize)):
            assert tuple(got) == want, r
    assert gpsiq.resample_span(2 ** 40, 0, 1 << 29) == (2 ** 43, 0)
    for bad in ((2 ** 60, 0, ONE), (10, 1 << 63, ONE), (10, 0, (1 << 29) - 1), (10, 0, (1 << 35) + 1), (10, 0, 0)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.resample_span(*bad)
        assert e.value.code == -1, bad
    assert gpsiq._resample_span(10, 0, ONE, None, None) == 0          # either result pointer may be NULL


def test_resample_step_round_trips_and_refusals():
    assert gpsiq.resample_step(2.6e6, 2.6e6) == ONE
    assert gpsiq.resample_step(2.6e6, 2.048e6) == round(ONE * 2.6 / 2.048) == STEPS[6]
    assert gpsiq.resample_step(2.6e6, 4.092e6) == round(ONE * 2.6 / 4.092)
    assert gpsiq.resample_step(8.0, 1.0) == 1 << 35 and gpsiq.resample_step(1.0, 8.0) == 1 << 29
    # a receiver whose clock runs fast takes more samples of the same signal: a smaller step
    for ppb in (-20000.0, -1.0, 1.0, 20000.0, 1e6):
        s = gpsiq.resample_step(3e6, 3e6, ppb)
        assert abs(s - ONE / (1 + ppb * 1e-9)) <= 0.5 + 1e-3 and (s < ONE) == (ppb > 0)
        # the step names the rate back: fs_out (1 + ppb 1e-9) = fs_in 2^32 / step to the step's own resolution
        assert abs(3e6 * ONE / s / 3e6 - (1 + ppb * 1e-9)) < 2.0 ** -32
    for bad in ((8.0001, 1.0, 0.0), (1.0, 8.0001, 0.0), (8.0, 1.0, -1000.0), (1.0, 8.0, 1000.0)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.resample_step(*bad)
        assert e.value.code == -2, bad
    for bad in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 1.0, 0.0), (float("inf"), 1.0, 0.0), (1.0, float("nan"), 0.0), (1.0, 1.0, float("inf")),
                (1.0, 1.0, -1e9)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.resample_step(*bad)
        assert e.value.code == -1, bad
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq._check(gpsiq._resample_step(1.0, 1.0, 0.0, None))


DESIGNS = [(STEPS[6], 0.8, 7, 16, 14), (ONE, 1.0, 8, 32, 14), (1 << 35, 0.9, 6, 64, 12), (1 << 29, 0.8, 5, 17, 8), (STEPS[7], 0.8, 0, 2, 14),
           (3 << 31, 0.5, 1, 9, 10), (STEPS[8], 0.7, 8, 7, 13)]


@pytest.mark.parametrize("step,bw,L,ntaps,shift", DESIGNS)
def test_resample_design_properties(step, bw, L, ntaps, shift):
    taps = gpsiq.resample_design(step, bw, L, ntaps, shift).astype(np.int64)
    nph = 1 << L
    assert taps.shape == (nph + 1, ntaps)
    assert (taps.sum(axis=1) == 1 << shift).all()                    # DC gain 1 at every phase
    assert int(np.abs(taps).sum(axis=1).max()) <= 65535 and int(np.abs(taps).max()) <= 32767
    # every row but row 0 ends in the zero of the vacated place
    assert (taps[1:, ntaps - 1] == 0).all()
    # row nphases - r is row r mirrored, to the bit; the one row that is its own mirror with two equal largest taps carries its
    # remainder (at most half a unit per tap) on the first of them
    for r in range(1, nph):
        a, b = taps[r, :ntaps - 1], taps[nph - r, :ntaps - 1][::-1]
        if 2 * r == nph and ntaps % 2 == 1:
            assert np.abs(a - b).max() <= ntaps / 2 and np.count_nonzero(a != b) <= 2
        else:
            assert np.array_equal(a, b), r
    # Row nphases is row 0 shifted by one tap.  Both are the same prototype values g(k + 1 - (ntaps-1)/2); row 0 has one value more,
    # g(-(ntaps-1)/2), in its sum S0 = SN + g0, so the scales differ by S0 / SN = 2^shift / (2^shift - row0[0]) up to the rounding of
    # row0[0] (half a unit).  Per tap: that ratio's share of the tap, one unit for the two roundings, and on each row's largest tap the
    # row's remainder, at most half a unit per tap.
    e = abs(int(taps[0, 0])) + 1
    ratio = e / ((1 << shift) - e)
    for k in range(ntaps - 1):
        tol = 1 + abs(int(taps[0, k + 1])) * ratio
        if k + 1 == int(np.argmax(taps[0])) or k == int(np.argmax(taps[nph])):
            tol += ntaps
        assert abs(int(taps[nph, k]) - int(taps[0, k + 1])) <= tol, (k, taps[nph], taps[0])
    # the formula itself, to a unit of rounding away from the largest tap
    w = bw * min(1.0, ONE / step)
    c = (ntaps - 1) / 2
    for r in (0, nph // 3, nph):
        t = np.arange(ntaps) + r / nph - c
        g = np.where(np.abs(t) <= c + 1e-12, np.sinc(w * t) * (0.54 + 0.46 * np.cos(2 * np.pi * t / (ntaps - 1))), 0.0)
        want = g / g.sum() * (1 << shift)
        dev = np.abs(taps[r] - want)
        big = int(np.argmax(dev))                                    # where the remainder went: a largest tap, the remainder at most half a unit per tap
        side = np.arange(ntaps) != big
        assert np.max(dev[side]) <= 0.5 + 1e-6 and dev[big] <= ntaps / 2 + 0.5 and (dev[big] <= 0.5 + 1e-6 or want[big] >= want.max() - 1.0), r


def test_resample_design_band_edges():
    """the cutoff follows the lower of the two rates: half amplitude at bandwidth * 0.5 * min(1, 2^32 / step) of the input rate"""
    for step, bw in ((STEPS[6], 0.8), (ONE, 0.8), (1 << 34, 0.8), (1 << 30, 0.6)):
        taps = gpsiq.resample_design(step, bw, 7, 32, 14).astype(np.float64)
        fc = bw * 0.5 * min(1.0, ONE / step)
        k = np.arange(32)
        resp = abs(np.sum(taps[0] * np.exp(-2j * np.pi * fc * k))) / (1 << 14)
        assert 0.45 <= resp <= 0.55, (step, resp)


def test_resample_design_refusals():
    ok = (STEPS[6], 0.8, 7, 16, 14)
    assert gpsiq.resample_design(*ok).shape == (129, 16)
    for bad in ((1 << 28, 0.8, 7, 16, 14), ((1 << 35) + 1, 0.8, 7, 16, 14), (ONE, 0.0, 7, 16, 14), (ONE, 1.01, 7, 16, 14), (ONE, -0.5, 7, 16, 14),
                (ONE, 0.8, -1, 16, 14), (ONE, 0.8, 9, 16, 14), (ONE, 0.8, 7, 1, 14), (ONE, 0.8, 7, 65, 14), (ONE, 0.8, 8, 64, 14), (ONE, 0.8, 8, 33, 14),
                (ONE, 0.8, 7, 16, 7), (ONE, 0.8, 7, 16, 15)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.resample_design(*bad)
        assert e.value.code == -1, bad
    assert gpsiq.resample_design(ONE, 0.8, 8, 32, 8).shape == (257, 32) and gpsiq.resample_design(ONE, 0.8, 6, 64, 14).shape == (65, 64)
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq._check(gpsiq._resample_design(ONE, 0.8, 7, 16, 14, None))


def test_calls_refuse_a_null_context_without_a_device():
    taps = np.zeros((2, 3), np.int16)
    n, nx, cl, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._resample(None, 16, SC08, None, None, gpsiq._p(taps), 0, 3, 0, 0, ONE, 0, SC08, None, None, C.byref(n), C.byref(nx), C.byref(cl),
                                     C.byref(ms)))
    assert e.value.code == -1 and "null context" in str(e.value)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._generate_batch_resampled(None, None, 1, 1, 16, 2.6e6, SC08, gpsiq._p(taps), 0, 3, 0, 0, ONE, 0, SC08, None, 64, C.byref(n),
                                                     C.byref(cl), None))
    assert e.value.code == -1
    out = (C.c_longlong * 4)()
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._resample_last_plan(None, out))
    assert e.value.code == -1


# ---- the planner ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_plans_hold_their_invariants_everywhere(sanitize):
    """Every request is held to the plan's own invariants inside the program (coverage of the outputs, table and window inside the LDS,
    grid inside its limit); here: the counts against the contract's formulas, nsamp up to the batch call's."""
    reqs = []
    for nsamp in (0, 1, 255, 256, 257, 511, 512, 513, 5000, 26_000_000, 2 ** 31 - 1):
        for L, ntaps in ((0, 1), (0, 64), (1, 2), (5, 7), (7, 16), (8, 32), (6, 64), (8, 1)):
            for step in STEPS:
                for pos0 in (0, ONE - 1, nsamp * ONE + 5):
                    for force in (rp.AUTO, rp.GENERIC, rp.ROWS):
                        reqs.append(("plan", nsamp, L, ntaps, step, pos0, force))
    lim = rp.ask([("limits",)], sanitize)[0]
    for r, p in zip(reqs, rp.ask(reqs, sanitize)):
        _, nsamp, L, ntaps, step, pos0, force = r
        assert (p.nout, p.next) == rr.span(nsamp, pos0, step), r
        if p.nout == 0:
            assert isinstance(p, rp.Nothing)
            continue
        want = {rp.GENERIC: 0, rp.ROWS: 1, rp.AUTO: lim.default}[force]
        assert p.kernel == want and p.run == (lim.run if want else lim.unit) and p.threads == lim.threads, r
        assert p.pad == (1 if want and step >= lim.pad_step else 0), r


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_grid_cap_pieces_and_the_most_a_piece_can_give(sanitize):
    lim = rp.ask([("limits",)], sanitize)[0]
    assert lim.threads == 256 and lim.run % lim.threads == 0 and lim.pad_step == 1 << 33 and rp.KERNELS[lim.default] in ("generic", "rows")
    # the grid is the units up to its cap, and the cap from there on
    for kernel, unit in ((rp.ROWS, lim.run), (rp.GENERIC, lim.unit)):
        a, b, c = rp.ask([("plan", unit * lim.max_grid - 1, 0, 1, ONE, 0, kernel), ("plan", unit * lim.max_grid, 0, 1, ONE, 0, kernel),
                          ("plan", unit * lim.max_grid + 1, 0, 1, ONE, 0, kernel)], sanitize)
        assert (a.grid, a.runs) == (lim.max_grid, lim.max_grid) and (b.grid, b.runs) == (lim.max_grid, lim.max_grid)
        assert (c.grid, c.runs) == (lim.max_grid, lim.max_grid + 1)
    got = rp.ask([("piece", 0, 4096, 8192, 0), ("piece", 7, 4096, 8192, 0), ("piece", 7, 4096, 8192, 3), ("piece", 7, 4096, 8192, 99),
                  ("piece", 4130, 260000, 520000, 0), ("piece", 100, 2 ** 31 - 1, 2 * (2 ** 31 - 1), 50), ("piece", 5000, 1 << 20, 1 << 21, 4000)], sanitize)
    assert got == [0, 7, 3, 7, 65, 1, 2047]                          # 32 MiB of source; a piece's samples fit an int whatever was asked
    # the staging of a piece holds its outputs whatever position it starts at
    reqs = [("most", n, s) for n in (1, 4096, 3 * 4096, 2 ** 31 - 1) for s in STEPS]
    for (_, n, s), most in zip(reqs, rp.ask(reqs, sanitize)):
        assert most == rr.span(n, 0, s)[0] and all(rr.span(n, p, s)[0] <= most for p in (1, ONE - 1, 5 * ONE))


# ---- gpsiq_runahead --resample: the checks that need no device ------------------------------------------------------------------------

def runahead(*flags, fs="2600000"):
    exe = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", fs, "2", "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--resample", "0"), ("--resample", "-2048000"), ("--resample", "abc"), ("--resample", "100000"),
                                   ("--resample", "30000000"), ("--resample", "2048000,x"), ("--resample", "2048000,-1e9"),
                                   ("--resample", "2048000", "--filter", "1.0e6"), ("--resample", "2048000", "--level", "2.3", "--pack", "4"),
                                   ("--resample", "2048000", "--tone", "100000,40")], ids=lambda f: " ".join(f))
def test_runahead_resample_refuses_what_the_stage_cannot_do(flags):
    r = runahead(*flags)                                             # (2.6 Msps: 100 ksps and 30 Msps are outside a ratio of 8)
    assert r.returncode == 2 and "usage:" in r.stderr and "--resample" in r.stderr, (r.returncode, r.stderr)


def test_runahead_resample_accepts_the_rest():
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--resample", "2048000"), ("--resample", "2.048e6,20000"), ("--resample", "4092000,-3500", "--cn0", "45"),
                  ("--resample", "2600000,20000", "--level", "2.3")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
