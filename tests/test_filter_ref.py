"""The filter stage on the CPU: tests/_filter_ref.py (the numpy restatement the GPU tests compare every byte with) against a second,
scalar statement of the contract of include/gpsiq_rows.h ("Filter"), continuation in pieces, the library's gpsiq_filter_span and
gpsiq_filter_design, the planner and the matrix operand of the calls (tests/filter_plan.cpp, also under ASan + UBSan), the refusals that need no device and
the argument checks of gpsiq_runahead --filter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _filter_plan as fp
import _filter_ref as fr
import gpsiq
from gpsiq.abi import SC08, SC16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
DESIGNS = [(10.4e6, 1.2e6, 65), (10.4e6, 1.0e6, 33), (2.6e6, 1.0e6, 31), (25e6, 2e6, 129), (5.2e6, 1.2e6, 17)]


def random_taps(rng, ntaps, total=None):
    """int16 taps of both signs; total: their sum of magnitudes exactly (at most 65535)"""
    t = rng.integers(-40, 41, size=ntaps).astype(np.int64)
    if total is not None:                                             # (three taps or more: two hold 65534 at the most)
        for k in range(ntaps):
            add = min(total - int(np.abs(t).sum()), 32767 - abs(int(t[k])))
            t[k] += add * (1 if t[k] >= 0 else -1)
        assert int(np.abs(t).sum()) == total and int(np.abs(t).max()) <= 32767
    return t.astype(np.int16)


# ---- the two statements of the contract -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("in_size", [SC08, SC16])
@pytest.mark.parametrize("out_size", [SC08, SC16])
def test_numpy_and_scalar_statements_agree(in_size, out_size):
    rng = np.random.default_rng(100 * in_size + out_size)
    clipped_somewhere = False
    for ntaps, decim, phase, nsamp, shift in [(1, 1, 0, 9, 0), (2, 2, 1, 17, 3), (7, 3, 2, 40, 5), (16, 4, 0, 33, 8), (17, 16, 15, 70, 14), (5, 3, 1, 1, 0),
                                             (9, 4, 3, 3, 24), (12, 1, 0, 50, 6)]:
        x = fr.full_range(rng, nsamp, in_size)
        head = fr.full_range(rng, ntaps - 1, in_size)
        taps = random_taps(rng, ntaps, 65535 if ntaps > 2 else None)
        for h in (None, head):
            a, ca = fr.filter_ref(x, h, taps, shift, decim, phase, out_size)
            b, cb = fr.filter_scalar(x, h, taps, shift, decim, phase, out_size)
            assert a.dtype == b.dtype and np.array_equal(a, b) and ca == cb and len(a) == fr.span(nsamp, decim, phase)[0]
            clipped_somewhere |= ca > 0
    assert clipped_somewhere


def test_rounding_and_clamp_by_hand():
    # one tap of 1: acc = x.  shift 1: floor((x + 1) / 2); -3 -> -1, 3 -> 2, -1 -> 0
    out, c = fr.filter_ref([[-3, 3], [-1, 1]], None, [1], 1, 1, 0, SC08)
    assert out.tolist() == [[-1, 2], [0, 1]] and c == 0
    # the clamp is symmetric and counted: 2 * -128 = -256 -> -127, 2 * 100 = 200 -> 127, 2 * 63 stays
    out, c = fr.filter_ref(np.array([[-128, 100], [63, -64]], np.int8), None, [2], 0, 1, 0, SC08)
    assert out.tolist() == [[-127, 127], [126, -127]] and c == 3
    # causal, with a head: y(0) = 3 x(0) + 5 x(-1)
    out, _ = fr.filter_ref([[10, -10]], [[1, 2]], [3, 5], 0, 1, 0, SC16)
    assert out.tolist() == [[35, -20]]


@pytest.mark.parametrize("decim", [1, 3, 4, 16])
def test_pieces_equal_the_whole(decim):
    rng = np.random.default_rng(decim)
    ntaps, nsamp, shift = 9, 131, 4
    x = fr.full_range(rng, nsamp, SC16)
    taps = random_taps(rng, ntaps)
    for phase in (0, decim - 1):
        whole, cw = fr.filter_ref(x, None, taps, shift, decim, phase, SC08)
        for cut in (1, ntaps - 2, ntaps - 1, nsamp // 2):
            hist = np.zeros((ntaps - 1, 2), np.int16)
            parts, clipped, ph = [], 0, phase
            for piece in (x[:cut], x[cut:cut + 5], x[cut + 5:]):      # the middle piece is shorter than the history
                o, c = fr.filter_ref(piece, hist, taps, shift, decim, ph, SC08)
                assert len(o) == fr.span(len(piece), decim, ph)[0]
                parts.append(o)
                clipped += c
                ph = fr.span(len(piece), decim, ph)[1]
                hist = np.concatenate([hist, piece])[len(piece):]
            assert np.array_equal(np.concatenate(parts), whole) and clipped == cw, (phase, cut)


# ---- the library's host arithmetic ------------------------------------------------------------------------------------------------

def test_filter_span_is_the_formulas():
    for nsamp in (0, 1, 2, 15, 16, 17, 1000, INT_MAX):
        for decim in (1, 2, 3, 4, 16):
            for phase in {0, decim - 1}:
                nout, nxt = gpsiq.filter_span(nsamp, decim, phase)
                assert (nout, nxt) == fr.span(nsamp, decim, phase)
                assert 0 <= nxt < decim or nout == 0
    for bad in ((-1, 1, 0), (10, 0, 0), (10, 17, 0), (10, 4, 4), (10, 4, -1)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.filter_span(*bad)
        assert e.value.code == -1


@pytest.mark.parametrize("fs,fc,ntaps", DESIGNS)
def test_filter_design_properties(fs, fc, ntaps):
    taps = gpsiq.filter_design(fs, fc, ntaps, 14).astype(np.int64)
    assert len(taps) == ntaps and np.array_equal(taps, taps[::-1]) and int(taps.sum()) == 1 << 14
    assert int(np.abs(taps).sum()) <= 65535
    k = np.arange(ntaps)
    resp = lambda f: abs(np.sum(taps * np.exp(-2j * np.pi * f / fs * k))) / (1 << 14)
    assert 0.49 <= resp(fc) <= 0.51, resp(fc)
    assert max(resp(f) for f in np.linspace(2 * fc, fs / 2, 200)) < 0.002 if 2 * fc < fs / 2 else True
    # the formula, to a step of the rounding (the centre tap also carries the remainder of the sum)
    w = 2 * fc / fs
    h = w * np.sinc(w * (k - (ntaps - 1) / 2)) * (0.54 - 0.46 * np.cos(2 * np.pi * k / (ntaps - 1)))
    want = h / h.sum() * (1 << 14)
    side = k != (ntaps - 1) // 2
    assert np.max(np.abs(taps[side] - want[side])) <= 0.5 + 1e-6 and abs(taps[~side][0] - want[~side][0]) <= ntaps / 2


def test_filter_design_refusals():
    for bad in ((10.4e6, 1.2e6, 64, 14), (10.4e6, 1.2e6, 1, 14), (10.4e6, 1.2e6, 513, 14), (10.4e6, 0.0, 65, 14), (10.4e6, 5.2e6, 65, 14),
                (10.4e6, -1.0, 65, 14), (10.4e6, 1.2e6, 65, 7), (10.4e6, 1.2e6, 65, 15), (0.0, 1.2e6, 65, 14)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.filter_design(*bad)
        assert e.value.code == -1, bad
    for shift in (8, 14):
        assert int(gpsiq.filter_design(10.4e6, 1.2e6, 65, shift).astype(np.int64).sum()) == 1 << shift


def test_calls_refuse_a_null_context_without_a_device():
    taps = np.array([1, 2, 1], np.int16)
    nout, clipped, ms = C.c_int(0), C.c_uint64(0), C.c_float(0)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._filter(None, 16, SC08, None, None, gpsiq._p(taps), 3, 0, 1, 0, SC08, None, None, C.byref(nout), C.byref(clipped), C.byref(ms)))
    assert e.value.code == -1 and "null context" in str(e.value)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._generate_batch_filtered(None, None, 1, 1, 16, 2.6e6, SC08, gpsiq._p(taps), 3, 0, 1, SC08, None, 64, C.byref(clipped), None))
    assert e.value.code == -1
    out = (C.c_long * 4)()
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._filter_last_plan(None, out))
    assert e.value.code == -1


# ---- the planner ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_plans_hold_their_invariants_everywhere(sanitize):
    """Every request is held to the plan's own invariants inside the program (coverage of the outputs, window inside the LDS, grid
    inside its limit); here: the counts against the contract's formulas, nsamp up to INT_MAX."""
    reqs = []
    for nsamp in (0, 1, 255, 256, 257, 1023, 1024, 1025, 5000, 26_000_000, 600_000_000, INT_MAX):
        for ntaps in (1, 2, 16, 17, 63, 64, 65, 129, 512):
            for decim in (1, 2, 3, 4, 16):
                for phase in {0, decim - 1}:
                    for in_size, force in ((SC08, fp.AUTO), (SC08, fp.GENERIC), (SC08, fp.MFMA), (SC16, fp.AUTO), (SC16, fp.MFMA)):
                        reqs.append(("plan", nsamp, in_size, ntaps, decim, phase, 1000, force))
    for r, p in zip(reqs, fp.ask(reqs, sanitize)):
        _, nsamp, in_size, ntaps, decim, phase, _, force = r
        assert (p.nout, p.next) == fr.span(nsamp, decim, phase), r
        if p.nout == 0:
            assert isinstance(p, fp.Nothing)
            continue
        if in_size == SC16 or force == fp.GENERIC:
            assert fp.KERNELS[p.kernel] == "generic", r              # the matrix kernel serves int8 inputs only
        if in_size == SC08 and force == fp.MFMA:
            assert fp.KERNELS[p.kernel] == "mfma", r


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_path_decision_on_both_sides_of_each_threshold(sanitize):
    lim = fp.ask([("limits",)], sanitize)[0]
    assert lim.max_tap == 127 * 256 + 127 and lim.threads == 256 and 1 < lim.min_taps <= 512
    ask = lambda *a: fp.KERNELS[fp.ask([("plan",) + a], sanitize)[0].kernel]
    # the measured threshold in taps, int8 input
    assert ask(10000, SC08, lim.min_taps - 1, 1, 0, 100, fp.AUTO) == "generic" and ask(10000, SC08, lim.min_taps, 1, 0, 100, fp.AUTO) == "mfma"
    assert ask(10000, SC16, lim.min_taps, 1, 0, 100, fp.AUTO) == "generic"
    # a tap that two signed bytes cannot hold goes to the generic kernel, forced or not
    for force in (fp.AUTO, fp.MFMA):
        assert ask(10000, SC08, 512, 4, 0, lim.max_tap, force) == "mfma" and ask(10000, SC08, 512, 4, 0, lim.max_tap + 1, force) == "generic"
    # forcing works below and above the threshold
    assert ask(10000, SC08, 1, 1, 0, 100, fp.MFMA) == "mfma" and ask(10000, SC08, 512, 1, 0, 100, fp.GENERIC) == "generic"
    # the run of a workgroup shrinks where the window would not fit, never below a workgroup's threads
    runs = {(nt, d): fp.ask([("plan", 10 ** 6, SC08, nt, d, 0, 100, f)], sanitize)[0].run for nt in (1, 65, 512) for d in (1, 16) for f in (fp.GENERIC,)}
    assert runs[(1, 1)] == runs[(65, 1)] == runs[(512, 1)] == lim.max_run and lim.threads <= runs[(512, 16)] < lim.max_run


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_pieces_tile_the_call_and_the_override_is_honoured(sanitize):
    got = fp.ask([("piece", 0, 4096, 8192, 0), ("piece", 7, 4096, 8192, 0), ("piece", 7, 4096, 8192, 3), ("piece", 7, 4096, 8192, 99),
                  ("piece", 4130, 260000, 520000, 0), ("piece", 100, INT_MAX, 2 * INT_MAX, 50), ("piece", 5000, 1 << 20, 1 << 21, 4000)], sanitize)
    assert got == [0, 7, 3, 7, 65, 1, 2047]                          # 32 MiB of source; a piece's samples fit an int whatever was asked


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_planes_times_window_is_the_direct_sum(sanitize):
    """filter_build_planes (csrc/gpsiq_filter_plan.h), the operand gpsiq_filter stages for filter_mfma: one tile column multiplied out
    in the kernel's arithmetic against the direct real sum, inside the program."""
    shapes = [(1, 1), (2, 1), (16, 1), (17, 3), (33, 1), (33, 16), (129, 4), (257, 2), (512, 1), (512, 16), (25, 7)]
    reqs = [("planes", ntaps, decim, seed, kind) for ntaps, decim in shapes for seed in (0, 1, 2) for kind in (0, 1)]
    assert all(fp.ask(reqs, sanitize))


# ---- gpsiq_runahead --filter: the checks that need no device -------------------------------------------------------------------------

def runahead(*flags, fs="10400000"):
    exe = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", fs, "2", "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--filter", "0"), ("--filter", "5200000"), ("--filter", "-3"), ("--filter", "1.2e6", "--taps", "64"),
                                   ("--filter", "1.2e6", "--taps", "1"), ("--filter", "1.2e6", "--taps", "513"), ("--filter", "1.2e6", "--decim", "0"),
                                   ("--filter", "1.2e6", "--decim", "17"), ("--filter", "1.2e6", "--decim", "3"), ("--taps", "65"), ("--decim", "4"),
                                   ("--filter", "1.2e6", "--level", "2.3", "--pack", "4"), ("--filter", "1.2e6", "--acquire"),
                                   ("--filter", "1.2e6", "--follow", "1", "--acquire")], ids=lambda f: " ".join(f))
def test_runahead_filter_refuses_what_the_stage_cannot_do(flags):
    r = runahead(*flags)                                              # (1 040 000 samples per block: 3 does not divide it)
    assert r.returncode == 2 and "usage:" in r.stderr and "--filter" in r.stderr and "--pack 4|2" in r.stderr, (r.returncode, r.stderr)


def test_runahead_filter_accepts_the_rest():
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--filter", "1.2e6"), ("--filter", "1.2e6", "--decim", "4"), ("--filter", "1e6", "--taps", "33", "--decim", "16", "--cn0", "45")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
