"""The spectrum stage on the CPU: tests/_spectrum_ref.py's matrix restatement (what the GPU tests compare every byte with) against its
scalar statement of the contract of include/gpsiq_rows.h ("Spectrum"), the span arithmetic, the bound and gpsiq_spectrum_min_shift,
gpsiq_spectrum_scale against its formula and against white noise, a table tone, the planner of the call (tests/spectrum_plan.cpp,
also under ASan + UBSan) and the refusals that need no device."""
import math
import os
import subprocess

import numpy as np
import pytest

import _spectrum_plan as sp
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16, WINDOW_HANN, WINDOW_RECT

INT_MAX = 2 ** 31 - 1
NFFT = [64, 128, 256, 512]
U64 = 2 ** 64 - 1


# ---- the two statements of the contract -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sample_size", [SC08, SC16])
@pytest.mark.parametrize("nfft", NFFT)
def test_matrix_and_scalar_statements_agree(sample_size, nfft):
    """every nfft, both hops, both windows, shift 0 and min_shift + 3; the scalar statement on bins at the edges and three in between"""
    rng = np.random.default_rng(10 * nfft + sample_size)
    bins = sorted({0, 1, nfft // 2 - 1, nfft // 2, nfft - 1} | set(int(k) for k in rng.integers(0, nfft, 2)))
    for hop in (nfft // 2, nfft):
        x = sr.full_range(rng, nfft + 4 * hop + 7, sample_size)      # five segments: two groups of two and one left over
        for window in (WINDOW_RECT, WINDOW_HANN):
            for shift in sorted({sr.min_shift(sample_size, nfft, window, 2), sr.min_shift(sample_size, nfft, window, 2) + 3}):
                a = sr.spectrum_ref(x, nfft, hop, window, 2, shift)
                b = sr.spectrum_scalar(x, nfft, hop, window, 2, shift, bins)
                assert a.shape == (2, nfft) and a.dtype == np.uint64
                assert all(int(a[g, k]) == v for (g, k), v in b.items()), (hop, window, shift)


def test_the_shift_floors_and_hann_is_the_three_bin_difference():
    # one sample of (1, 0) at n = 0: Xi[k] = c(0) = 250, Xq[k] = -s(0) = -2 for every bin; rect at shift 0: power = c(0)^2 + s(0)^2
    c, s = sr.table()
    x = np.zeros((64, 2), np.int8)
    x[0] = (1, 0)
    p = sr.spectrum_ref(x, 64, 64, WINDOW_RECT, 1, 0)
    assert (p == int(c[0]) ** 2 + int(s[0]) ** 2).all()
    # every bin equal: the Hann difference is zero everywhere
    assert (sr.spectrum_ref(x, 64, 64, WINDOW_HANN, 1, 0) == 0).all()
    # -s(0) = -2 is negative: shifted by 2 it floors to -1, not 0; c(0) = 250 >> 2 = 62
    assert int(c[0]) == 250 and int(s[0]) == 2
    assert (sr.spectrum_ref(x, 64, 64, WINDOW_RECT, 1, 2) == 62 * 62 + 1).all()


# ---- span arithmetic --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", NFFT)
def test_span_arithmetic_at_the_edges(nfft):
    for hop in (nfft // 2, nfft):
        for nsamp, nseg in [(0, 0), (nfft - 1, 0), (nfft, 1), (nfft + hop - 1, 1), (nfft + hop, 2), (nfft + 6 * hop + 3, 7)]:
            for navg in (1, 2, 3, 7, 8):
                assert gpsiq.spectrum_span(nsamp, nfft, hop, navg) == (nseg, nseg // navg) == sr.span(nsamp, nfft, hop, navg)
    assert gpsiq.spectrum_span(INT_MAX, nfft, nfft // 2, 1)[0] == (INT_MAX - nfft) // (nfft // 2) + 1
    for bad in [(-1, nfft, nfft, 1), (100, nfft + 1, nfft, 1), (100, nfft, nfft // 4, 1), (100, nfft, nfft, 0), (100, 1024, 1024, 1), (100, 32, 32, 1)]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.spectrum_span(*bad)
        assert e.value.code == -1


# ---- the bound --------------------------------------------------------------------------------------------------------------------

# (sample size, nfft, window, navg) -> shift.  int8, 512, Hann: Ymax = 4 * 512 * 500 * 128 = 2^17 * 1000, (2^64 - 1) / (2 Ymax^2) = 536.87.
# int8, 512, rect: Ymax = 2^15 * 1000, 8589.9.  int8, 64, Hann: Ymax = 2^14 * 1000, 34359.7.  int16, 64, rect: Ymax = 2^20 * 1000, 8.39.
# int16, 512, Hann: Ymax = 2^25 * 1000 = 3.36e10 > 2^32: no navg fits at shift 0; at shift 4 Ys = 2 097 152 001 and navg up to 2 fits,
# navg 3 does not (2 * 3 * Ys^2 = 2.64e19 > 1.84e19).
PINS = [(SC08, 512, 1, 536, 0), (SC08, 512, 1, 537, 1), (SC08, 512, 0, 8589, 0), (SC08, 512, 0, 8590, 1), (SC08, 64, 1, 34359, 0), (SC08, 64, 1, 34360, 1),
        (SC16, 64, 0, 8, 0), (SC16, 64, 0, 9, 1), (SC16, 64, 1, 1, 1), (SC16, 512, 0, 1, 2), (SC16, 512, 1, 1, 4), (SC16, 512, 1, 2, 4), (SC16, 512, 1, 3, 5),
        (SC16, 512, 1, INT_MAX, 19), (SC08, 64, 0, 1, 0)]


def test_min_shift_pins():
    asked = sp.ask([("minshift", ss, n, w, na) for ss, n, w, na, _ in PINS])
    for (ss, n, w, na, shift), planner in zip(PINS, asked):
        assert gpsiq.spectrum_min_shift(ss, n, w, na) == shift == planner == sr.min_shift(ss, n, w, na), (ss, n, w, na)
        assert sr.fits(ss, n, w, na, shift) and (shift == 0 or not sr.fits(ss, n, w, na, shift - 1))
    for bad in [(3, 512, 1, 1), (SC08, 100, 1, 1), (SC08, 512, 2, 1), (SC08, 512, 1, 0)]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.spectrum_min_shift(*bad)
        assert e.value.code == -1


def test_min_shift_agrees_with_the_restatement_over_a_sweep():
    cases = [(ss, n, w, na) for ss in (SC08, SC16) for n in NFFT for w in (0, 1) for na in (1, 2, 3, 10, 100, 537, 10 ** 4, 10 ** 6, 10 ** 8, INT_MAX)]
    for (ss, n, w, na), planner in zip(cases, sp.ask([("minshift",) + c for c in cases])):
        assert planner == sr.min_shift(ss, n, w, na) == gpsiq.spectrum_min_shift(ss, n, w, na)


@pytest.mark.parametrize("sample_size", [SC08, SC16])
def test_an_adversarial_span_stays_below_the_bound_and_the_bound_is_not_slack(sample_size):
    """Signs chosen against bin 1's twiddles at full scale.  The restatement itself asserts that cells and sums stay inside uint64.
    Slack, rectangular window: every term of Xi[1] is |c| xmax' + |s| xmax' with xmax' >= xmax - 1, so Xi[1] >= (xmax - 1) * sum over
    the table of (|c| + |s|) * N / 512, and the table's mean |c| + |s| is 250 * 4 / pi = 318.3 less its rounding (>= 318 - 1); the
    bound takes 500.  So Ymax^2 / Xi[1]^2 <= (500 / 317)^2 * (128 / 127)^2 = 2.53 < 2.6: the bound is slack by less than 2.6 in power,
    1.3 bits of the 64."""
    c, s = sr.table()
    assert float(np.abs(c).mean() + np.abs(s).mean()) >= 317.0
    for nfft in (64, 512):
        navg = 5
        x = sr.adversarial(sample_size, nfft, navg, nfft)
        for window in (WINDOW_RECT, WINDOW_HANN):
            shift = sr.min_shift(sample_size, nfft, window, navg)
            p = sr.spectrum_ref(x, nfft, nfft, window, navg, shift)
            assert int(p.max()) <= U64
            if window == WINDOW_RECT:
                ys = sr.ymax(sample_size, nfft, 0) >> shift
                assert int(p[0, 1]) * 2.6 >= navg * ys * ys, (nfft, int(p[0, 1]), navg * ys * ys)
        # one navg past the bound at shift 0 is refused by the arithmetic the call uses
        top = U64 // (2 * sr.ymax(sample_size, nfft, 1) ** 2)
        if top >= 1:
            assert sr.fits(sample_size, nfft, 1, top, 0) and not sr.fits(sample_size, nfft, 1, top + 1, 0)
            assert sp.ask([("fits", sample_size, nfft, 1, top, 0), ("fits", sample_size, nfft, 1, top + 1, 0)]) == [True, False]


# ---- the scale --------------------------------------------------------------------------------------------------------------------

def test_scale_against_its_formula():
    for nfft in NFFT:
        for window, G in ((0, 1.0), (1, 6.0)):
            for navg, shift, fs in [(1, 0, 2.6e6), (537, 1, 10.4e6), (10 ** 6, 40, 25e6), (3, 7, 1.0)]:
                want = 4.0 ** shift / (navg * 250.0 ** 2 * G * nfft * fs)
                assert math.isclose(gpsiq.spectrum_scale(nfft, window, navg, shift, fs), want, rel_tol=1e-12)
    for bad in [(100, 0, 1, 0, 1e6), (64, 2, 1, 0, 1e6), (64, 0, 0, 0, 1e6), (64, 0, 1, 41, 1e6), (64, 0, 1, -1, 1e6), (64, 0, 1, 0, 0.0), (64, 0, 1, 0, float("inf"))]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.spectrum_scale(*bad)
        assert e.value.code == -1


def test_the_hann_window_of_the_contract_has_gain_six():
    for nfft in NFFT:
        w = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)
        assert math.isclose(float((w * w).sum()), 6.0 * nfft, rel_tol=1e-12)


@pytest.mark.parametrize("window", [WINDOW_RECT, WINDOW_HANN])
def test_white_noise_reads_two_sigma_squared_over_fs(window):
    """Seeded Gaussian int16 streams, sigma 1000 (rounding adds 1/12 to the variance: 1e-7 relative).  A periodogram cell of white
    noise is exponentially distributed, its standard deviation equal to its mean; the mean over the N bins of M averaged segments
    therefore has a relative standard deviation of at most 1 / sqrt(M) (the bins of a Hann spectrum are correlated, so the N bins are
    not counted as independent), and the margin is six of those."""
    fs, sigma, nfft, M = 10.4e6, 1000.0, 256, 400
    rng = np.random.default_rng(2024 + window)
    x = np.rint(rng.normal(0.0, sigma, size=(nfft * M, 2))).astype(np.int16)
    shift = sr.min_shift(SC16, nfft, window, M)
    p = sr.spectrum_ref(x, nfft, nfft, window, M, shift)
    density = p[0].astype(np.float64) * gpsiq.spectrum_scale(nfft, window, M, shift, fs)
    want = 2.0 * sigma * sigma / fs
    rel = abs(float(density.mean()) / want - 1.0)
    print(f"window {window}: mean density / (2 sigma^2 / fs) - 1 = {rel:.4f}, margin {6 / math.sqrt(M):.4f}")
    assert rel <= 6.0 / math.sqrt(M)


@pytest.mark.parametrize("window", [WINDOW_RECT, WINDOW_HANN])
@pytest.mark.parametrize("nfft", NFFT)
def test_a_table_tone_peaks_in_its_bin(nfft, window):
    for k0 in (0, 1, nfft // 4 + 1, nfft // 2, nfft - 1):
        x = sr.table_tone(nfft, k0, 2, nfft // 2)
        p = sr.spectrum_ref(x, nfft, nfft // 2, window, 2, 0)
        assert int(np.argmax(p[0])) == k0, (k0, int(np.argmax(p[0])))


# ---- the planner ------------------------------------------------------------------------------------------------------------------

def test_kernel_choice_on_both_sides_of_every_threshold():
    lim = sp.limits()
    default = "mfma" if lim.default_mfma else "generic"
    for nfft in NFFT:
        for hop in (nfft // 2, nfft):
            nsamp = nfft + 99 * hop
            assert sp.KERNELS[sp.plan(nsamp, SC08, nfft, hop, 10).kernel] == default
            assert sp.KERNELS[sp.plan(nsamp, SC08, nfft, hop, 10, sp.GENERIC).kernel] == "generic"
            assert sp.KERNELS[sp.plan(nsamp, SC08, nfft, hop, 10, sp.MFMA).kernel] == "mfma"
            for force in (sp.AUTO, sp.GENERIC, sp.MFMA):                # int16 has no matrix path: forced or not, the generic kernel
                assert sp.KERNELS[sp.plan(nsamp, SC16, nfft, hop, 10, force).kernel] == "generic"
            # no whole group: nothing, whatever is forced
            assert sp.plan(nfft - 1, SC08, nfft, hop, 1, sp.MFMA) == sp.Nothing(0, 0)
            assert sp.plan(nfft + hop, SC08, nfft, hop, 3, sp.MFMA) == sp.Nothing(2, 0)


def test_grids():
    lim = sp.limits()
    # generic: a unit is up to `run` segments of one group; the grid is the units, capped
    p = sp.plan(512 + 999 * 512, SC16, 512, 512, 130)
    assert (p.nseg, p.ngroups, p.run, p.per, p.work, p.grid, p.threads) == (1000, 7, lim.run, 3, 21, 21, 256)
    assert sp.plan(64 + 999 * 64, SC16, 64, 64, 1).threads == 64 and sp.plan(128 + 128, SC16, 128, 128, 1).threads == 128
    big = sp.plan(INT_MAX, SC16, 64, 32, 1)
    assert big.nseg == (INT_MAX - 64) // 32 + 1 and big.work == big.ngroups == big.nseg and big.grid == lim.max_grid
    assert big.power_bytes == big.ngroups * 64 * 8
    # matrix kernel: a pass is 64 segments, 32 where 64 would not fit the LDS window (nfft 512 without overlap); a workgroup takes a
    # contiguous range of passes, and the grid stays at or below mfma_grid
    assert sp.plan(512 + 999 * 512, SC08, 512, 512, 1, sp.MFMA).run == 32
    for nfft, hop in [(512, 256), (256, 256), (256, 128), (128, 128), (64, 32), (64, 64)]:
        assert sp.plan(nfft + 999 * hop, SC08, nfft, hop, 1, sp.MFMA).run == 64
    p = sp.plan(64 + 99 * 64, SC08, 64, 64, 3, sp.MFMA)                # 100 segments, 33 groups, 99 read: two passes
    assert (p.nseg, p.ngroups, p.work, p.per, p.grid, p.threads) == (100, 33, 2, 1, 2, 256)
    big = sp.plan(INT_MAX, SC08, 64, 32, 1, sp.MFMA)
    assert big.work == (big.nseg + 63) // 64 and big.grid <= lim.mfma_grid and big.grid * big.per >= big.work > (big.grid - 1) * big.per


def test_planner_under_the_sanitizers_over_the_corner_arguments():
    reqs = []
    for ss in (SC08, SC16):
        for nfft in NFFT:
            for hop in (nfft // 2, nfft):
                for nsamp in (0, 1, nfft - 1, nfft, nfft + hop - 1, nfft + hop, 10 ** 6 + 1, INT_MAX - 1, INT_MAX):
                    for navg in (1, 3, 64, 65, 536, 537, INT_MAX):
                        for force in (sp.AUTO, sp.GENERIC, sp.MFMA):
                            reqs.append(("plan", nsamp, ss, nfft, hop, navg, force))
                for window in (0, 1):
                    for navg in (1, 536, 537, 8589, 8590, INT_MAX):
                        reqs.append(("minshift", ss, nfft, window, navg))
                        for shift in (0, 1, 39, 40):
                            reqs.append(("fits", ss, nfft, window, navg, shift))
    assert sp.ask(reqs, sanitize=True) == sp.ask(reqs)


# ---- gpsiq_runahead --spectrum: the checks that need no device ----------------------------------------------------------------------

def runahead(*flags):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", "10400000", "1", "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--spectrum", "0"), ("--spectrum", "100"), ("--spectrum", "1024"), ("--spectrum", "-64"),
                                   ("--spectrum", "512", "--level", "2.3", "--pack", "4")], ids=lambda f: " ".join(f))
def test_runahead_spectrum_refuses_what_the_stage_cannot_do(flags):
    r = runahead(*flags)
    assert r.returncode == 2 and "usage:" in r.stderr and "--spectrum" in r.stderr, (r.returncode, r.stderr)


def test_runahead_spectrum_accepts_the_rest():
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--spectrum", "64"), ("--spectrum", "512", "--cn0", "45"), ("--spectrum", "256", "--filter", "1.2e6", "--decim", "4"),
                  ("--spectrum", "128", "--acquire")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
