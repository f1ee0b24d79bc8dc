"""gpsiq_agc without a device: the host arithmetic of the library (gpsiq_agc_mult, gpsiq_agc_span: include/gpsiq_rows.h, "AGC") against
tests/_agc_ref.py's restatement with Python integers, the restatement's own continuation property, worked examples by hand, and every
range error of the contract that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import _agc_ref as ar
import gpsiq
from gpsiq.abi import SC08, SC16


def lib_mult(c, S, n):
    return gpsiq.agc_mult(ar.to_lib_cfg(c), S, n)


def test_gain_rule_at_its_edges():
    c = ar.cfg(target_q8=210, mult0=4321, mult_min=1, mult_max=(1 << 24) - 1)
    # n = 0: mult0, whatever the sum
    assert lib_mult(c, 0, 0) == 4321 == ar.mult(c, 0, 0)
    # S = 0: r is clamped to 1, the multiplier is target << 16 under its clamp
    assert lib_mult(c, 0, 128) == ar.mult(c, 0, 128) == min(210 << 16, (1 << 24) - 1)
    assert lib_mult(ar.cfg(target_q8=1, mult_max=(1 << 24) - 1), 0, 2) == 65536
    # all -32768: S = n * 2^30, m = 2^46, r = 2^23: the rms of 32768 in 1/256 units
    for n in (2, 128, 1 << 17, 1 << 23):
        assert lib_mult(c, n << 30, n) == ar.mult(c, n << 30, n) == (210 << 16) >> 23
    # n = 2^23 with the largest sum, and sums around it
    for S in ((1 << 53), (1 << 53) - 1, (1 << 52) + 12345, 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1):
        assert lib_mult(c, S, 1 << 23) == ar.mult(c, S, 1 << 23), S
    # both clamps
    lo = ar.cfg(target_q8=210, mult0=5000, mult_min=5000, mult_max=6000)
    assert lib_mult(lo, 2 << 30, 2) == ar.mult(lo, 2 << 30, 2) == 5000               # the rule gives 1
    assert lib_mult(lo, 0, 2) == ar.mult(lo, 0, 2) == 6000                           # the rule gives 210 << 16
    # the worked example: sigma 40 at target 210 is 65536 * (210 / 256) / 40 = 1344
    assert lib_mult(c, 1600 * 2048, 2048) == ar.mult(c, 1600 * 2048, 2048) == 1344


def test_gain_rule_on_random_pairs():
    rng = np.random.default_rng(11)
    cfgs = [ar.cfg(target_q8=int(t), mult0=int(m0), mult_min=int(lo), mult_max=int(hi))
            for t, lo, m0, hi in ((210, 1, 65536, (1 << 24) - 1), (1, 1, 1, 1), ((1 << 23) - 1, 1, 7, (1 << 24) - 1), (54, 300, 300, 70000), (1792, 16, 99, 1 << 20))]
    libs = [ar.to_lib_cfg(c) for c in cfgs]
    for i in range(4000):
        n = int(rng.integers(1, (1 << 23) + 1)) if i % 3 else int(rng.integers(1, 300))
        bits = int(rng.integers(0, 31))
        S = int(rng.integers(0, (n << bits) + 1)) if i % 5 else n << bits          # mean squares over the whole range, exact squares too
        k = i % len(cfgs)
        assert gpsiq.agc_mult(libs[k], S, n) == ar.mult(cfgs[k], S, n), (cfgs[k], S, n)
    # the square root is the floor one, either side of perfect squares
    c = ar.cfg(target_q8=(1 << 23) - 1, mult_max=(1 << 24) - 1)
    for r in (1, 2, 3, 255, 256, 4095, 65535, (1 << 23) - 1):
        for m in (r * r - 1, r * r, r * r + 1):
            if m >= 1:
                # m = S * 2^16 / n with n = 2^16: S = m
                assert gpsiq.agc_mult(ar.to_lib_cfg(c), m, 1 << 16) == min(max(((1 << 23) - 1 << 16) // max(math.isqrt(m), 1), 1), (1 << 24) - 1)


def test_gain_rule_refusals():
    good = ar.cfg()
    assert lib_mult(good, 5, 2) > 0
    for kw in (dict(target_q8=0), dict(target_q8=1 << 23), dict(mult_min=0), dict(mult_min=70000, mult0=70000, mult_max=69999), dict(mult_max=1 << 24),
               dict(mult0=0), dict(mult0=5, mult_min=6), dict(mult0=9, mult_max=8)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            lib_mult(good._replace(**kw), 5, 2)
        assert e.value.code == -1, kw
    for S, n in (((1 << 53) + 1, 1 << 23), (0, (1 << 23) + 1)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            lib_mult(good, S, n)
        assert e.value.code == -1
    m = C.c_uint32(0)
    assert gpsiq._agc_mult(None, 0, 0, C.byref(m)) == -1
    assert gpsiq._agc_mult(C.byref(ar.to_lib_cfg(good)), 0, 0, None) == -1


def test_span_is_the_formulas_and_refuses_the_rest():
    for W in (64, 128, 192, 1024, 65536):
        for fill in (0, 1, W // 2, W - 1):
            for n in (0, 1, W - fill - 1, W - fill, W - fill + 1, W, 700, 5 * W + 3, 2 ** 31 - 1, 2 ** 40 + 17):
                if n < 0:
                    continue
                assert gpsiq.agc_span(n, W, fill) == ar.span(n, W, fill), (n, W, fill)
    assert gpsiq.agc_span(0, 64, 63) == (0, 63)                      # no sample: no window touched, the fill stays
    for n, W, fill in ((10, 63, 0), (10, 0, 0), (10, 100, 0), (10, 65536 + 64, 0), (10, 64, 64), (10, -64, 0), (1 << 60, 64, 0)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.agc_span(n, W, fill)
        assert e.value.code == -1, (n, W, fill)
    assert gpsiq._agc_span(100, 64, 0, None, None) == 0              # either result may be NULL


@pytest.mark.parametrize("in_size,out_size", [(SC08, SC08), (SC16, SC08), (SC16, SC16)])
def test_one_call_equals_every_split_of_a_700_sample_span(in_size, out_size):
    rng = np.random.default_rng(5 + in_size)
    x = ar.full_range(rng, 700, in_size) // 4                        # a quarter of the range: below the threshold ...
    for at in (50, 51, 200, 330, 397, 699):                          # ... but for these (two of them hold + 2 apart)
        x[at] = ar.full_range(rng, 2, in_size)[at % 2]
    thresh = 100 if in_size == SC08 else 20000
    c = ar.cfg(window=128, navg=3, target_q8=900 if out_size == SC08 else 200000, mult0=3000, blank_thresh=thresh, blank_hold=65,
               qmax=5 if out_size == SC08 else 300)
    start = ar.State(((1000000, 200), (50, 256)), 777, 60, 31, 40)
    whole = ar.agc_ref(x, c, start, out_size)
    assert whole[1] > 0 and 0 < whole[2] < 700 and len(set(whole[3])) > 2
    for cut in range(0, 701):
        got = ar.in_pieces(x, c, [cut], start, out_size)
        assert np.array_equal(got[0], whole[0]) and got[1:] == whole[1:], cut
    # and a few cuts at once, pieces shorter than the hold among them
    for cuts in ([1, 2, 3], [97, 98, 130], [10, 40, 41, 600], [128 - 31, 256 - 31], [699]):
        got = ar.in_pieces(x, c, cuts, start, out_size)
        assert np.array_equal(got[0], whole[0]) and got[1:] == whole[1:], cuts


def test_blanker_and_gain_by_hand():
    """window 64, navg 2: three windows of constant (3, 4) -- power 25 a sample -- with one pulse; every number worked out by hand"""
    x = np.tile(np.array([[3, 4]], np.int16), (200, 1))
    x[70] = (0, 1000)
    c = ar.cfg(window=64, navg=2, target_q8=256 * 5, mult0=65536, blank_thresh=500, blank_hold=3, qmax=7)
    out, clipped, blanked, mults, st = ar.agc_ref(x, c, ar.FRESH, SC08)
    # window 0: mult0.  Mean square per element 25 / 2: r = isqrt(12.5 * 65536) = 905; 1280 << 16 // 905 = 92691 from window 1 on
    assert mults == [65536, 92691, 92691, 92691] and blanked == 4
    assert st == ar.State(((60 * 25, 120), (64 * 25, 128)), 8 * 25, 16, 8, 0)
    assert (out[70:74] == 0).all() and out[69].tolist() == [4, 6] and out[74].tolist() == [4, 6] and out[0].tolist() == [3, 4]
    assert clipped == 0
    # a pulse at the span's last sample leaves the whole hold; at the last but two, hold - 2
    for at, left in ((199, 3), (197, 1), (196, 0)):
        y = np.tile(np.array([[3, 4]], np.int16), (200, 1))
        y[at] = (-501, 0)
        assert ar.agc_ref(y, c, ar.FRESH, SC08)[4].hold == left
    # the clamp counts elements of unblanked samples only
    c1 = c._replace(qmax=4)
    out, clipped, _, _, _ = ar.agc_ref(x, c1, ar.FRESH, SC08)
    assert clipped == 200 - 64 - 4 and out[100].tolist() == [4, 4]   # from window 1 on the 6 becomes 4; the pulse's 1000 is blanked, not counted


def test_device_calls_refuse_without_a_device_what_needs_none():
    """a null context; every range of the configuration and an impossible state are checked before the device is touched, so a context
    that was never created shows the order: the configuration's error comes first only where the context is there -- here the null
    context's"""
    cfg = ar.to_lib_cfg(ar.cfg())
    cl, bl, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._agc(None, 16, SC08, None, C.byref(cfg), None, SC08, None, None, None, C.byref(cl), C.byref(bl), C.byref(ms)))
    assert e.value.code == -1 and "null context" in str(e.value)
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._generate_batch_agc(None, None, 1, 1, 16, 2.6e6, SC08, C.byref(cfg), None, SC08, None, 64, C.byref(cl), C.byref(bl), None))
    assert e.value.code == -1
    out = (C.c_longlong * 6)()
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq._check(gpsiq._agc_last_plan(None, out))
    assert e.value.code == -1


def test_structures_have_the_layout_of_the_header():
    assert C.sizeof(gpsiq.AgcCfg) == 36 and C.sizeof(gpsiq.AgcState) == 64 * 8 + 64 * 4 + 8 + 4 * 4
    assert gpsiq.AgcState.psum.offset == 768 and gpsiq.AgcState.hold.offset == 788
    s = ar.State(((5, 2), (7, 4)), 9, 2, 1, 0)
    assert ar.from_lib_state(ar.to_lib_state(s)) == s and ar.from_lib_state(gpsiq.AgcState()) == ar.FRESH


# ---- gpsiq_runahead --agc / --blank: the checks that need no device ------------------------------------------------------------------

def runahead(*flags, ss="1"):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", "2600000", ss, "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--agc", "0"), ("--agc", "2.3"), ("--agc", "2.3,0"), ("--agc", "2.3,128"), ("--agc", "2.3,7,100,4"), ("--agc", "2.3,7,1024"),
                                   ("--agc", "2.3,7,1024,0"), ("--agc", "2.3,7,1024,65"), ("--agc", "2.3,7,131072,4"), ("--agc", "40000,7"), ("--agc", "2.3,7x"),
                                   ("--blank", "90,64"), ("--agc", "2.3,7", "--blank", "0,64"), ("--agc", "2.3,7", "--blank", "90"),
                                   ("--agc", "2.3,7", "--blank", "90,1025"), ("--agc", "2.3,7", "--blank", "40000,4"), ("--agc", "2.3,7", "--agc", "2.3,7"),
                                   ("--agc", "2.3,7", "--level", "2.3", "--pack", "4"), ("--agc", "2.3,7", "--filter", "1.0e6"), ("--agc", "2.3,7", "--tone", "100000,40"),
                                   ("--agc", "2.3,7", "--resample", "2048000")], ids=lambda f: " ".join(f))
def test_runahead_agc_refuses_what_the_stage_cannot_do(flags):
    r = runahead(*flags)
    assert r.returncode == 2 and "usage:" in r.stderr and "--agc" in r.stderr, (r.returncode, r.stderr)


def test_runahead_agc_accepts_the_rest():
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--agc", "2.3,7"), ("--agc", "0.9,1,4096,4"), ("--agc", "2.3,127,64,64", "--blank", "90,0"), ("--agc", "2.3,7", "--blank", "32767,1024", "--cn0", "45"),
                  ("--agc", "2.3,7", "--level", "30", "--seed", "5"), ("--agc", "2.3,7", "--spectrum", "256")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
    assert runahead("--agc", "9000,32767", ss="2").returncode == 1 and runahead("--agc", "9000,32767").returncode == 2      # the clamp has to fit the format
