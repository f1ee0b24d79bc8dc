"""gpsiq_acquire on the CPU: the numpy restatement (tests/_acquire_ref.py) pinned by a case computed by hand, the digit decomposition
of the matrix path over every value of both formats, gpsiq_acquire_steps and gpsiq_acquire_decide against their formulas, the planner
(tests/acquire_plan.cpp over csrc/gpsiq_acquire_plan.h, also built with the address and undefined-behaviour sanitizers), the argument
checks of gpsiq_runahead --acquire, and the loop closed on the reference alone: a block rendered by the oracle at a set C/N0 is
searched by the restatement, which finds the satellites that are there where they are and no others.  tests/test_gpu_acquire.py
repeats that case on the device and must match its integers."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _acquire_plan as ap
import _acquire_ref as ar
import _despread_ref as dr
import _noise_ref as nr
import _oracle
import gpsiq
from gpsiq.abi import SC08, SC16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def test_a_stream_that_is_the_code_times_a_quarter_cycle_carrier(orc):
    """ncoh 64, PRN 5, one chip and a quarter of a cycle per sample: the carrier index of sample m is 128 (m mod 4), where the table
    holds (cos, sin) = (250, 2), (-2, 250), (-250, -2), (2, -250).  With I = ca * cos and Q = ca * sin, yi = ca (cos^2 + sin^2) =
    62 504 ca and yq = 0, so at shift 0 Xi = 64 * 62 504 = 4 000 256, Xq = 0 and the power is 4 000 256^2 = 16 002 048 065 536."""
    s, c = orc.tables()
    assert [(int(c[k]), int(s[k])) for k in (0, 128, 256, 384)] == [(250, 2), (-2, 250), (-250, -2), (2, -250)]
    code_step, step, ncoh, nshift = 1 << 56, 1 << 57, 64, 8
    chips = orc.codegen(5).astype(np.int64)
    assert np.array_equal(ar.sampled_code(orc, 5, code_step, ncoh), 1 - 2 * chips[:64])
    n = ncoh + nshift - 1
    ca = 1 - 2 * chips[:n]
    idx = 128 * (np.arange(n) % 4)
    assert np.array_equal(ar.carrier_index(step, n), idx)
    stream = np.stack([ca * c[idx], ca * s[idx]], axis=1).astype(np.int16).ravel()
    peaks, power, corr = ar.acquire(orc, stream, [5], code_step, step, 0, 1, nshift, ncoh)
    assert (int(corr["i"][0, 0, 0, 0]), int(corr["q"][0, 0, 0, 0])) == (4000256, 0)
    assert power[0, 0, 0] == 16002048065536.0 and peaks["shift"][0, 0] == 0 and peaks["power"][0, 0] == 16002048065536.0
    # every other cell, sample by sample in Python integers
    for sft in range(1, nshift):
        assert ar.acquire_direct(orc, stream, 5, code_step, step, sft, 0, ncoh, ncoh) == (int(corr["i"][0, 0, 0, sft]), int(corr["q"][0, 0, 0, sft]))
    assert power[0, 0, 1:].max() < power[0, 0, 0] / 4


def test_the_matrix_product_equals_the_sum_written_out(orc):
    """random int16 bytes, two dwells with a hop that is no multiple of anything, a negative step: cells picked across the grid"""
    rng = np.random.default_rng(12)
    nshift, ncoh, nn, hop, ndopp = 37, 128, 2, 77, 3
    stream = rng.integers(-32768, 32768, size=2 * ap.span_of(nshift, ncoh, nn, hop)).astype(np.int16)
    code_step, c0, ci = ar.steps(2.6e6, -1000.0, 1000.0)
    peaks, power, corr = ar.acquire(orc, stream, [3, 31], code_step, c0, ci, ndopp, nshift, ncoh, nn, hop)
    for p, d, k, s in [(0, 0, 0, 0), (1, 2, 1, 36), (0, 1, 1, 17), (1, 0, 0, 5)]:
        assert ar.acquire_direct(orc, stream, (3, 31)[p], code_step, c0 + d * ci, s, k, hop, ncoh) == (int(corr["i"][p, d, k, s]), int(corr["q"][p, d, k, s]))
    xi, xq = corr["i"].astype(np.float64), corr["q"].astype(np.float64)
    want = (0.0 + (xi[:, :, 0] * xi[:, :, 0] + xq[:, :, 0] * xq[:, :, 0])) + (xi[:, :, 1] * xi[:, :, 1] + xq[:, :, 1] * xq[:, :, 1])
    assert np.array_equal(power, want) and np.array_equal(peaks["shift"], power.argmax(axis=2))


# ---- the digit planes of the matrix path --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,nd", [(np.int8, 3), (np.int16, 4)])
def test_every_value_times_the_extreme_table_entries_reconstructs_from_its_digits(orc, dtype, nd):
    """y = I rI + Q rQ and Q rI - I rQ for EVERY value of the format as I, with Q at either extreme and equal to I, at the table entries
    where |cos| + |sin| is largest (354, within the 355 the planes are sized for) and where one of them is 250: balanced base-256 digits in [-128, 127] that sum back to y, with
    nothing left over; -128 and -32768 go through"""
    s, c = orc.tables()
    mag = np.abs(s) + np.abs(c)
    top = int(mag.max())
    assert top == 354                                         # 250 sqrt 2 = 353.6 on the table's own grid
    idx = np.unique(np.concatenate([np.flatnonzero(mag == top), np.flatnonzero(np.abs(s) == 250)[:4], np.flatnonzero(np.abs(c) == 250)[:4]]))
    info = np.iinfo(dtype)
    v = np.arange(info.min, info.max + 1, dtype=np.int64)
    bound = -info.min * top
    seen = 0
    for q in (np.full_like(v, info.min), np.full_like(v, info.max), v, -np.maximum(v, info.min + 1)):
        for k in idx:
            for y in (v * c[k] + q * s[k], q * c[k] - v * s[k]):
                dg, left = ar.digits(y, nd)
                assert not left.any() and dg.min() >= -128 and dg.max() <= 127
                assert np.array_equal(sum(dg[i] << (8 * i) for i in range(nd)), y)
                assert np.abs(y).max() <= bound
                seen = max(seen, int(np.abs(y).max()))
    assert seen == bound                                      # the bound is reached, by the most negative value at both inputs
    # one digit fewer does not hold the range (why int16 takes four planes and int8 three)
    assert ar.digits(np.array([bound, -bound]), nd - 1)[1].any()


def test_digit_ranges():
    """three balanced digits hold [-8 421 504, 8 355 711]: enough for 128 * 355, not for 32768 * 355"""
    lo, hi = -128 * (1 + 256 + 65536), 127 * (1 + 256 + 65536)
    assert (lo, hi) == (-8421504, 8355711) and 128 * 355 <= hi < 32768 * 355
    for y in (lo, hi, 0, -1, 127, 128, -128, -129):
        dg, left = ar.digits(np.array([y]), 3)
        assert not left.any() and int(sum(int(dg[i, 0]) << (8 * i) for i in range(3))) == y
    assert ar.digits(np.array([hi + 1]), 3)[1].any() and ar.digits(np.array([lo - 1]), 3)[1].any()


# ---- the helpers ----------------------------------------------------------------------------------------------------------------------

def test_acquire_steps_equal_the_formulas():
    for fs, f0, df in ((2.6e6, -5000.0, 500.0), (25e6, 0.0, 250.0), (4.092e6, 1234.5, -333.25), (2.6e6, 0.0, 0.0), (1.0e6, -499999.0, 1.0)):
        assert gpsiq.acquire_steps(fs, f0, df) == ar.steps(fs, f0, df)
    code, c0, ci = gpsiq.acquire_steps(2.6e6, -5000.0, 500.0)
    assert code == int(np.rint(1.023e6 / 2.6e6 * 2.0 ** 56)) and c0 == -10 * ci + (c0 + 10 * ci) and abs(c0 + 10 * ci) <= 5


@pytest.mark.parametrize("args,code", [((2.6e6, 1.3e6, 500.0), -2), ((2.6e6, 0.0, -1.3e6), -2), ((2.6e6, -1.4e6, 0.0), -2), ((0.5e6, 0.0, 0.0), -2),
                                       ((1e-9, 0.0, 0.0), -2), ((0.0, 0.0, 0.0), -1), ((-1.0, 0.0, 0.0), -1), ((float("nan"), 0.0, 0.0), -1),
                                       ((float("inf"), 0.0, 0.0), -1), ((2.6e6, float("nan"), 0.0), -2)])
def test_acquire_steps_refuse(args, code):
    """|f / fs| of a half and more, a code step of two chips per sample and more (fs <= 511.5 kHz): GPSIQ_E_RANGE; a bad fs: GPSIQ_E_ARG"""
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.acquire_steps(*args)
    assert e.value.code == code, str(e.value)


def test_acquire_steps_at_the_edges_of_the_ranges():
    assert gpsiq.acquire_steps(511501.0, 0.0, 0.0)[0] < 1 << 57
    assert gpsiq.acquire_steps(2.6e6, 1.2999e6, -1.2999e6)[1] < 1 << 58


def test_acquire_decide_equals_the_rule():
    rng = np.random.default_rng(3)
    for nd, ns, guard in ((1, 9, 0), (3, 40, 3), (21, 260, 3), (2, 5, 1), (4, 8, 6)):
        g = rng.random((nd, ns))
        for _ in range(4):
            g[rng.integers(nd), rng.integers(ns)] = rng.integers(2, 9)
            want = ar.decide(g, guard)
            if want is None:                                         # the peak so placed that the guard covers every shift
                with pytest.raises(gpsiq.GpsiqError):
                    gpsiq.acquire_decide(g, guard)
            else:
                assert gpsiq.acquire_decide(g, guard) == want
    # ties: the lowest bin, then the lowest shift; the floor is looked for in EVERY bin, the peak's own shift +- guard excluded in all
    g = np.ones((3, 10))
    g[1, 7] = g[1, 2] = g[2, 0] = 5.0
    assert gpsiq.acquire_decide(g, 1) == (1, 2, 1.0)                 # the floor is the other 5.0 at shift 7 (and 0)
    g[0, 2] = 5.0
    assert gpsiq.acquire_decide(g, 1)[:2] == (0, 2)
    g = np.ones((2, 12))
    g[1, 5], g[0, 6], g[0, 9] = 8.0, 4.0, 2.0
    assert gpsiq.acquire_decide(g, 0) == (1, 5, 2.0) and gpsiq.acquire_decide(g, 1) == (1, 5, 4.0) and gpsiq.acquire_decide(g, 4) == (1, 5, 8.0)
    # no wrap-around: shift 0 and shift 11 are 11 apart
    g = np.ones((1, 12))
    g[0, 0], g[0, 11] = 9.0, 3.0
    assert gpsiq.acquire_decide(g, 2) == (0, 0, 3.0)


@pytest.mark.parametrize("grid,guard,code", [(np.ones((2, 5)), 4, -2), (np.ones((1, 1)), 0, -2), (np.array([[3.0, 0.0, 0.0, 0.0]]), 1, -2),
                                             (np.zeros((2, 6)), 1, -2), (np.ones((2, 5)), -1, -1), (np.ones((0, 5)), 1, -1), (np.ones((2, 0)), 1, -1)])
def test_acquire_decide_refuses(grid, guard, code):
    """no cell outside the guard, or only zeros there: GPSIQ_E_RANGE; an empty grid or a negative guard: GPSIQ_E_ARG"""
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.acquire_decide(grid, guard)
    assert e.value.code == code, str(e.value)
    if code == -2:
        assert ar.decide(grid, guard) is None


# ---- planner --------------------------------------------------------------------------------------------------------------------------

def case_requests(force):
    return [(ap.span_of(c.nshift, c.ncoh, c.nnoncoh, c.hop), c.ss, len(c.prns), c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop, force) for c in ap.CASES]


def test_every_case_takes_the_kernels_it_is_written_for():
    forced, generic, plain = ap.query_many(case_requests("mfma")), ap.query_many(case_requests("generic")), ap.query_many(case_requests(None))
    default_fast = ap.query(30000, SC08, 32, 41, 2600, 2560, 1, 2600).kernel == "mfma"
    for c, f, g, d in zip(ap.CASES, forced, generic, plain):
        span = ap.span_of(c.nshift, c.ncoh, c.nnoncoh, c.hop)
        assert f.kernel == "mfma" and g.kernel == "generic", (c.name, f, g)
        assert d.kernel == ("mfma" if default_fast and ap.full_tile(c.ndopp, c.nshift) else "generic"), (c.name, d)
        assert f.digits == (3 if c.ss == SC08 else 4) and f.row_tiles == (c.ndopp + 1) // 2 and f.ksteps == c.ncoh // 64 + 5
        assert f.span == span and f.npad >= span and f.scratch == 16 * f.row_tiles * f.npad and f.lds == 16 * (c.ncoh + 48)
        assert (f.mx, f.my, f.mz) == (-(-c.nshift // 256), -(-f.row_tiles // 4), len(c.prns))
        assert (g.gx, g.gy, g.gz) == (-(-c.nshift // 256), c.ndopp, len(c.prns)) and g.scratch == 0
        assert f.cells == len(c.prns) * c.ndopp * c.nshift and f.corr_cells == f.cells * c.nnoncoh
    # the table reaches both digit counts, partly filled and full row tiles, one and several blocks of 256 shifts, on both kernels
    assert {(f.digits, c.ndopp % 2, f.mx > 1) for c, f in zip(ap.CASES, forced)} >= {(3, 0, False), (3, 1, True), (4, 0, True), (4, 1, False)}


def test_planner_rules():
    # the workload's own shape: 32 satellites, 41 bins, 2600 shifts, 1 ms at 2.6 Msps, 10 dwells
    p = ap.query(2600 + 9 * 2600 + 2560, SC08, 32, 41, 2600, 2560, 10, 2600, "mfma")
    assert (p.kernel, p.digits, p.row_tiles, p.ksteps, p.lds) == ("mfma", 3, 21, 45, 41728) and (p.mx, p.my, p.mz) == (11, 6, 32)
    assert p.npad == 2560 + 23392 + 2560 + 320 and p.scratch == 21 * 16 * p.npad
    # the knob beats the default either way; what the matrix path cannot serve is generic whatever is asked
    assert ap.query(5000, SC16, 1, 2, 256, 3072, 1, 1, "mfma").kernel == "mfma"
    assert ap.query(5000, SC16, 1, 2, 256, 3136, 1, 1, "mfma").kernel == "generic"                  # the code copies would not fit the LDS
    assert ap.query(INT_MAX, SC16, 1, 1024, 600000, 64, 1, 1, "mfma").kernel == "generic"          # 512 tiles x 16 x 600 384 bytes: above the cap
    assert ap.query(INT_MAX, SC16, 1, 1024, 30000, 64, 1, 1, "mfma").kernel == "mfma"
    assert ap.query(30000, SC08, 32, 41, 2600, 2560, 1, 2600, "nofast").kernel == "generic"
    for shape in ((30000, SC08, 4, 1, 2600, 2560, 1, 2600), (30000, SC08, 4, 2, 255, 2560, 1, 2600)):
        assert ap.query(*shape).kernel == "generic" and ap.query(*shape, "mfma").kernel == "mfma"  # below a full tile: only on request
    # not a search
    ok = (1000, SC16, 2, 3, 100, 128, 2, 200)
    assert ap.query(*ok) is not None and ap.span_of(100, 128, 2, 200) == 427
    for i, bad in ((0, 426), (1, 0), (1, 4), (2, 0), (2, 33), (3, 0), (3, 1025), (4, 0), (5, 0), (5, 32), (5, 100), (5, (1 << 20) + 64), (6, 0), (7, 0), (0, -1)):
        assert ap.query(*(ok[:i] + (bad,) + ok[i + 1:])) is None, (i, bad)
    assert ap.query(427, *ok[1:]) is not None


def test_planner_under_the_sanitizers():
    """the same table, and sizes next to INT_MAX and next to the argument limits, through the program built with
    -fsanitize=address,undefined: a program of its own, host code only"""
    for force in ("mfma", "generic", None):
        assert ap.query_many(case_requests(force), sanitize=True) == ap.query_many(case_requests(force))
    big = [(INT_MAX, SC16, 32, 1024, INT_MAX - (1 << 20) + 1, 1 << 20, 1, INT_MAX, None),           # the longest span there is
           (INT_MAX, SC16, 32, 1024, 1, 1 << 20, 2048, 1023, "mfma"),
           (INT_MAX, SC08, 32, 1024, 1, 64, INT_MAX // 2 - 40, 2, "mfma"),
           (INT_MAX, SC08, 1, 1, INT_MAX - 63, 64, 1, INT_MAX, "mfma"),
           (INT_MAX, SC08, 32, 1024, INT_MAX - 63, 64, 1, 1, "generic"),
           (INT_MAX, SC08, 32, 1024, 2, 64, INT_MAX, INT_MAX, None),                                 # (nnoncoh - 1) * hop next to 2^62: not a search
           (INT_MAX, SC16, 1, 2, 16384, 3072, 1000, 2000, "mfma")]
    got = ap.query_many(big, sanitize=True)
    assert got == ap.query_many(big)
    assert got[0].kernel == "generic" and got[0].span == INT_MAX and got[0].cells == 32 * 1024 * (INT_MAX - (1 << 20) + 1) and got[0].gx == 8384512
    assert got[1].kernel == "generic" and got[2].kernel == "generic" and got[2].span == 2 * (INT_MAX // 2 - 41) + 64
    assert got[3].kernel == "generic" and got[4].corr_cells == got[4].cells and got[5] is None and got[6].kernel == "mfma"


# ---- gpsiq_runahead --acquire: the checks that need no device -----------------------------------------------------------------------

def runahead(*flags, fs="2600000"):
    exe = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", fs, "1", "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


def test_runahead_acquire_argument_checks():
    """--acquire takes no value, searches the rendered elements (so not with --pack) and needs a millisecond of 64 samples or more and
    five of them in a block; a well-formed line gets past the checks and stops at the RINEX file that is not there"""
    for flags in (("--level", "2.3", "--pack", "4", "--acquire"), ("--acquire", "--level", "2.3", "--pack", "4")):
        r = runahead(*flags)
        assert r.returncode == 2 and "usage:" in r.stderr and "--acquire" in r.stderr, (flags, r.returncode, r.stderr)
    r = runahead("--acquire", fs="60000")
    assert r.returncode == 2 and "--acquire" in r.stderr, (r.returncode, r.stderr)
    for flags in (("--acquire",), ("--cn0", "45", "--level", "42", "--acquire"), ("--acquire", "--cn0", "45"), ("--cn0", "45", "--acquire", "--seed", "3")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)


# ---- the loop closed on the reference -------------------------------------------------------------------------------------------------

# The four ratios (best cell over the largest cell more than 3 samples from its shift, gpsiq_acquire_decide) as tests/_acquire_ref.py
# measures them on the oracle's block, in the order searched: present satellites 7 and 19, absent 3 and 28.  Arithmetic on the dwell
# statistics said 6-8 against 1.0-1.4; PRN 7 comes out lower because its code edge lies at sample 12.62, between two shifts.
# The decision threshold is the geometric mean of the smallest present and the largest absent ratio: sqrt(4.5472 * 1.0892).
MEASURED = [4.5472, 5.5859, 1.0029, 1.0892]
THRESHOLD = 2.2255


@functools.lru_cache(maxsize=None)
def loop_reference():
    """(descriptors CHAN_DTYPE [2], noisy int16 stream of LOOP's first block with both satellites on, steps, peaks, power, corr)"""
    L, S = dr.LOOP, ar.SEARCH
    orc = _oracle.load_oracle()
    d = ar.loop_descriptors()
    q, _ = gpsiq.quantize_blocks(d, L["fs"], L["nsamp"])
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    z = nr.noise(L["seed"], sigma, 0, 1, L["nsamp"])
    stream = nr.add_noise16(orc.block_fixed(q[0], L["nsamp"], SC16)[None, :], z)[0]
    st = gpsiq.acquire_steps(L["fs"], S["f0"], S["df"])
    return (d[0], stream, st) + ar.acquire(orc, stream, S["prns"], *st, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])


def test_a_blind_search_finds_the_two_satellites_that_were_rendered_and_no_others():
    L, S = dr.LOOP, ar.SEARCH
    d, stream, st, peaks, power, corr = loop_reference()
    assert ap.span_of(S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"]) <= L["nsamp"] and tuple(d["prn"]) == S["prns"][:2]
    got = [gpsiq.acquire_decide(power[p], S["guard"]) for p in range(4)]
    for p in range(4):
        print(f"PRN {S['prns'][p]}: bin {got[p][0]} ({S['f0'] + got[p][0] * S['df']:.0f} Hz), shift {got[p][1]}, ratio {got[p][2]:.4f}")
        assert got[p] == ar.decide(power[p], S["guard"])
        b = int(np.argmax(peaks["power"][p]))
        assert (b, int(peaks["shift"][p, b])) == got[p][:2]
    for p in range(2):                                                  # the present ones: where the descriptor says
        want_bin, want_shift = ar.expected_cell(d[p], L["fs"])
        print(f"PRN {S['prns'][p]}: f_carr {d[p]['f_carr']:.1f} Hz -> bin {want_bin}, code reaches chip 0 at sample {want_shift:.2f}")
        assert got[p][0] == want_bin and abs(got[p][1] - want_shift) <= 1.0, (got[p], want_bin, want_shift)
    present, absent = min(got[0][2], got[1][2]), max(got[2][2], got[3][2])
    assert present >= 2.0 * absent, (present, absent)
    assert MEASURED is not None and [round(g[2], 4) for g in got] == MEASURED
    assert THRESHOLD == pytest.approx(np.sqrt(present * absent), rel=1e-3) and absent < THRESHOLD < present
