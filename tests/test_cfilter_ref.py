"""gpsiq_cfilter without a device: the two statements of the contract (tests/_cfilter_ref.py) against each other, by hand and against
the real filter's restatement (the two identities of include/gpsiq_rows.h, "Complex filter and notch"); continuation; what the host
refuses without a device; the library's host arithmetic gpsiq_notch_find against the restatement in Python integers and
gpsiq_notch_design against its three properties; and the notch chain of tests/test_gpu_notch_signal.py on the restatements alone."""
import ctypes as C
import math

import numpy as np
import pytest

import _cfilter_ref as cr
import _filter_ref as fr
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16


def random_ctaps(rng, ntaps, total=None):
    """[ntaps, 2] int16 of both signs in both components; total: the sum of |re| + |im| exactly (at most 65535)"""
    t = rng.integers(-40, 41, size=2 * ntaps).astype(np.int64)
    if total is not None:
        for k in range(2 * ntaps):
            add = min(total - int(np.abs(t).sum()), 32767 - abs(int(t[k])))
            t[k] += add * (1 if t[k] >= 0 else -1)
        assert int(np.abs(t).sum()) == total
    return t.astype(np.int16).reshape(-1, 2)


# ---- the two statements of the contract -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_size", [SC08, SC16])
@pytest.mark.parametrize("out_size", [SC08, SC16])
def test_numpy_and_scalar_statements_agree(in_size, out_size):
    rng = np.random.default_rng(200 * in_size + out_size)
    clipped_somewhere = False
    for ntaps, decim, phase, nsamp, shift in [(1, 1, 0, 9, 0), (2, 2, 1, 17, 3), (7, 3, 2, 40, 5), (16, 4, 0, 33, 8), (17, 16, 15, 70, 14), (5, 3, 1, 1, 0),
                                             (9, 4, 3, 3, 24), (12, 1, 0, 50, 6), (70, 1, 0, 30, 9)]:
        x = cr.full_range(rng, nsamp, in_size)
        head = cr.full_range(rng, ntaps - 1, in_size)
        taps = random_ctaps(rng, ntaps, 65535 if ntaps > 1 else None)
        for h in (None, head):
            a, ca = cr.cfilter_ref(x, h, taps, shift, decim, phase, out_size)
            b, cb = cr.cfilter_scalar(x, h, taps, shift, decim, phase, out_size)
            assert a.dtype == b.dtype and np.array_equal(a, b) and ca == cb and len(a) == cr.span(nsamp, decim, phase)[0]
            clipped_somewhere |= ca > 0
    assert clipped_somewhere


def test_arithmetic_by_hand():
    # (3 + 4j)(10 - 20j) = 30 + 80 + j (40 - 60) = 110 - 20j
    out, c = cr.cfilter_ref([[10, -20]], None, [[3, 4]], 0, 1, 0, SC16)
    assert out.tolist() == [[110, -20]] and c == 0
    # causal, with a head: y(0) = h0 x(0) + h1 x(-1) = (1 + 2j)(5 + 6j) + (0 - 1j)(7 - 8j) = (-7 + 16j) + (-8 - 7j)
    out, _ = cr.cfilter_ref([[5, 6]], [[7, -8]], [[1, 2], [0, -1]], 0, 1, 0, SC16)
    assert out.tolist() == [[-15, 9]]
    # shift 1 rounds half up, the clamp is symmetric and counted: j * (-128 + 100j) = -100 - 128j -> (-100, -127)
    out, c = cr.cfilter_ref(np.array([[-128, 100]], np.int8), None, [[0, 1]], 0, 1, 0, SC08)
    assert out.tolist() == [[-100, -127]] and c == 1
    out, c = cr.cfilter_ref([[-3, 3]], None, [[1, 0]], 1, 1, 0, SC08)
    assert out.tolist() == [[-1, 2]] and c == 0


@pytest.mark.parametrize("in_size", [SC08, SC16])
def test_the_two_identities(in_size):
    rng = np.random.default_rng(5 + in_size)
    x = cr.full_range(rng, 300, in_size)
    for ntaps, decim, phase, shift in [(1, 1, 0, 0), (9, 3, 2, 7), (33, 1, 0, 14)]:
        re = rng.integers(-900, 901, size=ntaps).astype(np.int16)
        head = cr.full_range(rng, ntaps - 1, in_size)
        for out_size in (SC08, SC16):
            want = fr.filter_ref(x, head, re, shift, decim, phase, out_size)
            got = cr.cfilter_ref(x, head, np.stack([re, np.zeros_like(re)], axis=1), shift, decim, phase, out_size)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    # multiplication by j: (-Q, I), and -(-32768) is clamped and counted
    x = x.copy()
    x[7, 1] = -128 if in_size == SC08 else -32768
    out, c = cr.cfilter_ref(x, None, [[0, 1]], 0, 1, 0, in_size)
    qmax = 127 if in_size == SC08 else 32767
    want = np.stack([-x[:, 1].astype(np.int64), x[:, 0].astype(np.int64)], axis=1)
    assert np.array_equal(out, np.clip(want, -qmax, qmax)) and c == int(np.count_nonzero(np.abs(want) > qmax)) and c >= 1


@pytest.mark.parametrize("decim", [1, 3])
def test_every_split_of_a_40_sample_span_continues_exactly(decim):
    rng = np.random.default_rng(40 + decim)
    ntaps, nsamp, shift = 9, 40, 4
    x = cr.full_range(rng, nsamp, SC16)
    taps = random_ctaps(rng, ntaps, 65535)
    for phase in range(decim):
        whole, cw = cr.cfilter_ref(x, None, taps, shift, decim, phase, SC08)
        for cut in range(nsamp + 1):
            for cut2 in {cut, min(cut + 3, nsamp)}:                   # two pieces, and three with a middle one shorter than the history
                hist = np.zeros((ntaps - 1, 2), np.int16)
                parts, clipped, ph = [], 0, phase
                for piece in (x[:cut], x[cut:cut2], x[cut2:]):
                    o, c = cr.cfilter_ref(piece, hist, taps, shift, decim, ph, SC08)
                    parts.append(o)
                    clipped += c
                    ph = cr.span(len(piece), decim, ph)[1]
                    hist = np.concatenate([hist, piece])[len(piece):]  # the head is taken from the pieces before
                assert np.array_equal(np.concatenate(parts), whole) and clipped == cw, (phase, cut, cut2)


# ---- the library without a device -------------------------------------------------------------------------------------------------

def test_the_call_refuses_a_null_context_without_a_device():
    taps = np.array([[1, 0], [2, 1]], np.int16)
    nout, clipped, ms = C.c_int(0), C.c_uint64(0), C.c_float(0)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._cfilter(None, 16, SC08, None, None, gpsiq._p(taps), 2, 0, 1, 0, SC08, None, None, C.byref(nout), C.byref(clipped), C.byref(ms)))
    assert e.value.code == -1 and "null context" in str(e.value)
    out = (C.c_long * 4)()
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq._check(gpsiq._cfilter_last_plan(None, out))


def test_the_binding_takes_taps_as_an_array_or_as_ctaps():
    want = np.array([[1, -2], [3, 4]], np.int16)
    assert np.array_equal(gpsiq.ctaps(want), want) and np.array_equal(gpsiq.ctaps([[1, -2], [3, 4]]), want)
    assert np.array_equal(gpsiq.ctaps([gpsiq.CTap(1, -2), gpsiq.CTap(3, 4)]), want)
    assert np.array_equal(gpsiq.ctaps((gpsiq.CTap * 2)(gpsiq.CTap(1, -2), gpsiq.CTap(3, 4))), want)
    assert C.sizeof(gpsiq.CTap) == 4
    for bad in (np.zeros(4, np.int16), np.zeros((2, 3), np.int16), [[1, 40000]]):
        with pytest.raises(gpsiq.GpsiqError):
            gpsiq.ctaps(bad)


# ---- gpsiq_notch_find --------------------------------------------------------------------------------------------------------------

def spectrum_with(nfft, floor, runs):
    """power [nfft]: `floor` everywhere (jittered below it in the lower half of the cells), runs: {first bin: [cells]} laid cyclically"""
    p = [floor - (k % 3) for k in range(nfft)]
    for k0, cells in runs.items():
        for d, v in enumerate(cells):
            p[(k0 + d) % nfft] = v
    return np.array(p, dtype=np.uint64)


def check_find(power, fs, ratio, max_lines):
    f, ex, n = gpsiq.notch_find(power, fs, ratio, max_lines)
    wf, wex, wn = cr.notch_find(power, fs, ratio, max_lines)
    assert n == wn and len(f) == len(wf) == min(n, max_lines)
    assert np.allclose(f, wf, rtol=0, atol=1e-9 * fs) and np.allclose(ex, wex, rtol=0, atol=1e-9)
    return f, ex, n


@pytest.mark.parametrize("nfft", [64, 128, 256, 512])
def test_notch_find_is_the_restatement(nfft):
    fs, floor = 2.6e6, 10 ** 9
    # a run that wraps from bin nfft - 1 to bin 0: symmetric about bin -0.5 ... here about 0 with three cells
    f, ex, n = check_find(spectrum_with(nfft, floor, {nfft - 1: [20 * floor, 900 * floor, 20 * floor]}), fs, 8.0, 8)
    assert n == 1 and abs(f[0]) < 1e-6 and abs(ex[0] - 10 * math.log10(900)) < 1e-7    # (the floor is the jittered median, floor - 1)
    f, _, n = check_find(spectrum_with(nfft, floor, {nfft - 2: [50 * floor, 50 * floor, 50 * floor, 50 * floor]}), fs, 8.0, 8)
    assert n == 1 and abs(f[0] + 0.5 * fs / nfft) < 1e-6                # bins -2 .. 1: the centroid is bin -0.5
    # a run across the Nyquist edge comes back inside [-fs / 2, fs / 2)
    f, _, n = check_find(spectrum_with(nfft, floor, {nfft // 2 - 1: [10 * floor, 90 * floor, 90 * floor]}), fs, 8.0, 8)
    assert n == 1 and -fs / 2 <= f[0] < -fs / 2 + fs / nfft
    # two runs, the stronger first whatever its bin; a single cell between them keeps them apart
    f, ex, n = check_find(spectrum_with(nfft, floor, {5: [30 * floor, 40 * floor], 8: [70 * floor]}), fs, 8.0, 8)
    assert n == 2 and abs(f[0] - 8 * fs / nfft) < 1e-6 and ex[0] > ex[1]
    # equal peaks: the lower first bin first
    f, _, n = check_find(spectrum_with(nfft, floor, {20: [70 * floor], 9: [70 * floor]}), fs, 8.0, 8)
    assert n == 2 and f[0] < f[1]
    # more lines than max_lines: the strongest max_lines of them, nlines counts all
    many = {3 * i + 1: [(10 + i) * floor] for i in range(11)}
    f, ex, n = check_find(spectrum_with(nfft, floor, many), fs, 8.0, 3)
    assert n == 11 and len(f) == 3 and abs(f[0] - 31 * fs / nfft) < 1e-6 and list(ex) == sorted(ex, reverse=True)
    # exactly at ratio x floor is not over; one above is
    p = spectrum_with(nfft, floor, {7: [8 * (floor - 1)]})            # the floor is the jittered median, floor - 1
    assert sorted(int(v) for v in p)[nfft // 2 - 1] == floor - 1
    assert check_find(p, fs, 8.0, 8)[2] == 0
    p[7] += 1
    assert check_find(p, fs, 8.0, 8)[2] == 1
    assert check_find(p, fs, 2.5, 1)[2] == 1


def test_notch_find_takes_the_lower_middle_cell_as_the_floor():
    # a tie at the median: 32 cells of 100, 32 of 1000 -- the floor is 100 (the lower middle), and the upper half is over at ratio 8
    p = np.array([100] * 32 + [1000] * 32, dtype=np.uint64)
    f, ex, n = check_find(p, 64.0, 8.0, 8)
    assert n == 1 and abs(ex[0] - 10.0) < 1e-9 and abs(f[0] - (-16.5)) < 1e-9      # bins 32 .. 63 = -32 .. -1
    p = np.array([100] * 33 + [1000] * 31, dtype=np.uint64)
    assert check_find(p, 64.0, 8.0, 8)[2] == 1
    p = np.array([100] * 31 + [1000] * 33, dtype=np.uint64)          # now the lower middle cell is 1000: nothing is over
    assert check_find(p, 64.0, 8.0, 8)[2] == 0
    # full-width cells keep their integer order
    top = 2 ** 64 - 1
    p = np.array([top // 9] * 40 + [top] * 24, dtype=np.uint64)
    assert check_find(p, 64.0, 8.0, 8)[2] == 1


def test_notch_find_refusals():
    good = spectrum_with(64, 1000, {5: [90000]})
    assert gpsiq.notch_find(good, 1e6, 8.0, 1)[2] == 1
    zero = good.copy()
    zero[:40] = 0
    assert cr.notch_find(zero, 1e6, 8.0, 8) is None
    for power, fs, ratio, mx in ((zero, 1e6, 8.0, 8), (good, 1e6, 1.0, 8), (good, 1e6, 0.5, 8), (good, 1e6, float("nan"), 8), (good, 1e6, 8.0, 0),
                                (good, 1e6, 8.0, 9), (good, 0.0, 8.0, 8), (good[:32], 1e6, 8.0, 8), (np.resize(good, 96), 1e6, 8.0, 8),
                                (np.resize(good, 1024), 1e6, 8.0, 8)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.notch_find(power, fs, ratio, mx)
        assert e.value.code == -1
    n = C.c_int(0)
    f = np.zeros(8)
    for args in ((None, 64, 1e6, 8.0, 8, gpsiq._p(f), gpsiq._p(f), C.byref(n)), (gpsiq._p(good), 64, 1e6, 8.0, 8, None, gpsiq._p(f), C.byref(n)),
                 (gpsiq._p(good), 64, 1e6, 8.0, 8, gpsiq._p(f), None, C.byref(n)), (gpsiq._p(good), 64, 1e6, 8.0, 8, gpsiq._p(f), gpsiq._p(f), None)):
        assert gpsiq._notch_find(*args) == -1


# ---- gpsiq_notch_design -----------------------------------------------------------------------------------------------------------

FS = 2.6e6
DESIGNS = [("dc", [0.0], 129), ("quarter", [FS / 4], 129), ("near -fs/2", [-FS / 2 + 3e3], 129),
           ("three at the width", [-40e3, 0.0, 40e3], 129), ("33 taps", [300e3], 33), ("511 taps", [300e3, -711e3], 511)]


@pytest.mark.parametrize("shift", [8, 14])
@pytest.mark.parametrize("name,lines,ntaps", DESIGNS, ids=[d[0] for d in DESIGNS])
def test_notch_design_properties(name, lines, ntaps, shift):
    width = 40e3 if ntaps != 33 else 160e3
    taps = gpsiq.notch_design(FS, lines, width, ntaps, shift).astype(np.int64)
    c = (ntaps - 1) // 2
    assert taps.shape == (ntaps, 2) and int(np.abs(taps).sum()) <= 65535
    # 1. linear phase
    assert np.array_equal(taps[c:, 0], taps[c::-1, 0]) and np.array_equal(taps[c:, 1], -taps[c::-1, 1])
    # 2. only rounding is left at a line
    rounding = 0.7072 * ntaps / (1 << shift)
    at_lines = np.abs(cr.response(taps, shift, lines, FS))
    assert at_lines.max() <= rounding, (at_lines, rounding)
    # 3. away from every line the gain is 1 to the prototype's stop band, weighted by the a_l, and the rounding
    g = cr.prototype(ntaps, width / 2 / FS)
    grid = np.linspace(-FS / 2, FS / 2, 4001)[:-1]
    away = width / 2 + 3.3 * FS / ntaps
    G = lambda f: np.abs(cr.response(np.stack([g, np.zeros_like(g)], axis=1) * float(1 << 20), 20, f, FS))      # |G(f)| of g itself
    cyc = lambda d: np.minimum(np.abs(d), FS - np.abs(d))
    g_stop = G(grid[cyc(grid) >= away]).max()
    om = 2 * np.pi * np.asarray(lines) / FS
    n = np.arange(ntaps) - c
    M = np.array([[np.sum(g * np.cos((a - b) * n)) for b in om] for a in om])
    a = np.linalg.solve(M, np.ones(len(lines)))
    if len(lines) == 1:
        assert abs(a[0] - 1.0) < 1e-12
    far = grid[np.all([cyc(grid - f) >= away for f in lines], axis=0)]
    assert len(far) > 100
    dev = np.abs(np.abs(cr.response(taps, shift, far, FS)) - 1.0)
    assert dev.max() <= np.abs(a).sum() * g_stop + rounding, (dev.max(), np.abs(a).sum(), g_stop, rounding)
    # the formula itself, to a step of the rounding
    h = -sum(al * g * np.exp(1j * w * n) for al, w in zip(a, om))
    h[c] += 1.0
    assert np.max(np.abs(taps[:, 0] - h.real * (1 << shift))) <= 0.5 + 1e-6 and np.max(np.abs(taps[:, 1] - h.imag * (1 << shift))) <= 0.5 + 1e-6


def test_notch_design_refusals_and_the_range_case():
    ok = dict(fs=FS, f_hz=[100e3], width_hz=40e3, ntaps=129, shift=12)
    assert gpsiq.notch_design(**ok).shape == (129, 2)
    for kw in (dict(ntaps=128), dict(ntaps=1), dict(ntaps=513), dict(shift=7), dict(shift=15), dict(f_hz=[]), dict(f_hz=[1e3 * i for i in range(9)]),
               dict(f_hz=[FS / 2]), dict(f_hz=[-FS / 2]), dict(f_hz=[100e3, 139e3]), dict(f_hz=[FS / 2 - 10e3, -FS / 2 + 10e3]), dict(width_hz=0.0),
               dict(fs=0.0), dict(f_hz=[float("nan")])):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.notch_design(**{**ok, **kw})
        assert e.value.code == -1, kw
    assert gpsiq.notch_design(**{**ok, "f_hz": [100e3, 140e3]}).shape == (129, 2)     # exactly the width apart
    # eight lines of 511 taps at shift 14: sum |re| + |im| is 66274 (GPSIQ_E_RANGE); the caller lowers the shift, and 13 serves
    eight = [-1.2e6, -0.83e6, -0.51e6, -0.2e6, 0.07e6, 0.33e6, 0.74e6, 1.1e6]
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.notch_design(FS, eight, 10e3, 511, 14)
    assert e.value.code == -2
    assert next(s for s in range(13, 7, -1) if _designs(eight, s)) == 13


def _designs(lines, shift):
    try:
        return int(np.abs(gpsiq.notch_design(FS, lines, 10e3, 511, shift).astype(np.int64)).sum()) <= 65535
    except gpsiq.GpsiqError as e:
        assert e.code == -2
        return False


# ---- the notch chain on the restatements: what tests/test_gpu_notch_signal.py then asks of the device, byte for byte ------------------

def spectrum_of(x):
    nseg, _ = sr.span(len(x), cr.NOTCH_NFFT, cr.NOTCH_HOP, 1)
    return sr.spectrum_ref(x, cr.NOTCH_NFFT, cr.NOTCH_HOP, 1, nseg, sr.min_shift(SC16, cr.NOTCH_NFFT, 1, nseg))[0]


@pytest.mark.parametrize("case", sorted(cr.NOTCH_CASES))
def test_the_notch_chain_on_the_restatements(case):
    """Seed 20261, sigma 200, amplitude 8000, ratio 8.  One tone: found at bin 37.00006 with an excess of 51.3 dB; after the notch the
    largest cell of the output's spectrum stands 3.4 times over its floor (1.5 times once the filter's start-up of 128 samples is left
    out), against the ratio of 8.  Two tones: bins 37.00006 and -90.00005 at 51.3 dB each, 3.2 times afterwards."""
    bins = cr.NOTCH_CASES[case]
    x = cr.notch_stream(bins)
    f, ex, n = gpsiq.notch_find(spectrum_of(x), cr.NOTCH_FS, cr.NOTCH_RATIO, 8)
    assert n == len(bins) and sorted(np.rint(f / cr.bin_hz(1)).astype(int)) == sorted(bins)
    assert np.max(np.abs(np.sort(f) - np.sort([cr.bin_hz(b) for b in bins]))) < 0.01 * cr.bin_hz(1) and ex.min() > 45.0
    taps = gpsiq.notch_design(cr.NOTCH_FS, f, cr.NOTCH_WIDTH_BINS * cr.bin_hz(1), cr.NOTCH_NTAPS, cr.NOTCH_SHIFT)
    y, clipped = cr.cfilter_ref(x, None, taps, cr.NOTCH_SHIFT, 1, 0, SC16)
    assert clipped == 0
    q = spectrum_of(y)
    assert gpsiq.notch_find(q, cr.NOTCH_FS, cr.NOTCH_RATIO, 8)[2] == 0 and cr.notch_find(q, cr.NOTCH_FS, cr.NOTCH_RATIO, 8)[2] == 0
    assert max(int(v) for v in q) < 4 * sorted(int(v) for v in q)[cr.NOTCH_NFFT // 2 - 1]      # with room: half the ratio
