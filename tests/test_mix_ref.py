"""The mix stage on the CPU: the numpy restatement (tests/_mix_ref.py) against a slow big-integer loop, continuation through
gpsiq.mix_advance, the identity, the host helpers' values and refusals, the planner (csrc/gpsiq_mix_plan.h through tests/mix_plan.cpp,
plain and sanitized), and the argument checks of gpsiq_runahead --tone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mix_plan as mp
import _mix_ref as mr
import gpsiq
from gpsiq.abi import MIX_MAX_TERMS, MIX_ROTATED, MIX_STREAM, MIX_TONE, SC08, SC16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_RANGE = -1, -2                        # GPSIQ_E_ARG, GPSIQ_E_RANGE (include/gpsiq.h)


def some_terms(rng, nsamp):
    """every kind, both formats, delays, sweeps, gates, negative step / rate / gain"""
    a, b = mr.full_range(rng, nsamp, SC08), mr.full_range(rng, nsamp, SC16)
    return [mr.Term(MIX_STREAM, 300, a),
            mr.Term(MIX_STREAM, -7, b, skip=5, gate=(3, 1, 2)),
            mr.Term(MIX_ROTATED, 2, b, skip=3, phase0=123 << 40, step=-(41 << 50) - 12345, rate=3 << 44, sweep=(7, 3)),
            mr.Term(MIX_ROTATED, -3, a, skip=0, step=(5 << 50) + 99, gate=(129, 64, 100)),
            mr.Term(MIX_TONE, 1000, phase0=2 ** 64 - 5, step=37 << 50, rate=-(1 << 45), sweep=(65, 64)),
            mr.Term(MIX_TONE, -2500, step=-(100 << 50), rate=1 << 30)]


@pytest.mark.parametrize("m0", [0, 1, 2 ** 32 - 40, 2 ** 40 + 1, 2 ** 64 - 30])
@pytest.mark.parametrize("shift,qmax,dtype", [(0, 32767, np.int16), (8, 127, np.int8), (11, 9000, np.int16)])
def test_the_restatement_agrees_with_the_slow_loop(m0, shift, qmax, dtype):
    rng = np.random.default_rng(7)
    nsamp = 71
    terms = some_terms(rng, nsamp)
    want, wc = mr.mix_slow(nsamp, m0, terms, shift, qmax, dtype)
    got, gc = mr.mix_ref(nsamp, m0, terms, shift, qmax, dtype)
    assert np.array_equal(got, want) and gc == wc
    assert gc > 0 or shift == 11                                       # the clamp is exercised where the sum is large


def test_the_sign_convention_and_the_chirp_step():
    """a tone of positive step turns counter-clockwise, and the step at sweep position r is step + r * rate"""
    cos, sin = mr.table()
    out, _ = mr.mix_ref(8, 0, [mr.Term(MIX_TONE, 1, step=64 << 50)], 0, 32767, np.int16)       # an eighth of a cycle per sample
    assert [tuple(v) for v in out[:3]] == [(cos[0], sin[0]), (cos[64], sin[64]), (cos[128], sin[128])]
    assert sin[128] > 0 and abs(cos[128]) < 5
    out, _ = mr.mix_ref(6, 0, [mr.Term(MIX_TONE, 1, step=1 << 50, rate=2 << 50, sweep=(4, 0))], 0, 32767, np.int16)
    # phases in table steps: m * 1 + tri(r) * 2 with r = m mod 4: 0, 1, 2 + 2, 3 + 6, 4 + 0, 5 + 0
    assert [tuple(v) for v in out] == [(cos[i], sin[i]) for i in (0, 1, 4, 9, 4, 5)]


@pytest.mark.parametrize("cut", [1, 4, 5, 6, 30, 70])
def test_continuation_through_mix_advance(cut):
    """pieces on each side of the delays (3 and 5 samples) give the bytes and the count of one call; gpsiq.mix_advance moves the
    library's terms as the restatement's move"""
    rng = np.random.default_rng(8)
    nsamp, m0 = 71, 2 ** 32 - 40
    terms = some_terms(rng, nsamp)
    want, wc = mr.mix_ref(nsamp, m0, terms, 8, 127, np.int8)
    later = [t.advanced(cut) for t in terms]
    a, ac = mr.mix_ref(cut, m0, terms, 8, 127, np.int8)
    b, bc = mr.mix_ref(nsamp - cut, m0 + cut, later, 8, 127, np.int8)
    assert np.array_equal(np.concatenate([a, b]), want) and ac + bc == wc
    base = 1 << 20
    moved = gpsiq.mix_advance([t.mixterm(0 if t.x is None else base) for t in terms], cut)
    for t, l, m in zip(terms, later, moved):
        assert m.skip == l.skip and m.kind == t.kind and m.gain == t.gain and m.step == t.step and m.rate == t.rate
        assert m.phase0 == t.phase0 % 2 ** 64 and (m.gate_period, m.gate_on, m.gate_offset) == t.gate and (m.sweep_period, m.sweep_offset) == t.sweep
        if t.x is None:
            assert m.src is None
        else:
            assert m.src == base + max(0, cut - t.skip) * 2 * t.sample_size


@pytest.mark.parametrize("ss,dtype,qmax", [(SC08, np.int8, 127), (SC16, np.int16, 32767), (SC16, np.int16, 100)])
def test_identity(ss, dtype, qmax):
    rng = np.random.default_rng(9)
    x = mr.full_range(rng, 300, ss)
    for shift in (0, 1, 13):
        out, clipped = mr.mix_ref(300, 5, [mr.Term(MIX_STREAM, 1 << shift, x)], shift, qmax, dtype)
        want = np.clip(x.astype(np.int64), -qmax, qmax)
        assert np.array_equal(out, want.astype(dtype)) and clipped == int(np.count_nonzero(want != x))


def test_mix_tone_values_and_refusals():
    fs = 2.6e6
    assert gpsiq.mix_tone(fs, 0.0) == (0, 0, 0)
    assert gpsiq.mix_tone(fs, fs / 8) == (2 ** 56, 0, 0)
    assert gpsiq.mix_tone(fs, -fs / 4) == (-(2 ** 57), 0, 0)
    step, rate, period = gpsiq.mix_tone(fs, -1e5, 5.5e5, 1e-3)
    assert period == 2600 and step == round(-1e5 / fs * 2 ** 59) and abs(rate - 6.5e5 / fs / 2600 * 2 ** 59) <= 1
    step, rate, period = gpsiq.mix_tone(1e6, 2e5, -2e5, 2e-6)
    assert period == 2 and rate == round(-4e5 / 1e6 / 2 * 2 ** 59)
    for bad, code in (((fs, fs / 2), "range"), ((fs, -fs / 2), "range"), ((fs, 0.0, fs / 2, 1e-3), "range"), ((fs, 0.0, 1e3, 1e-7), "range"),
                      ((fs, 0.0, 1e3, 1e6), "range"), ((0.0, 1.0), "arg"), ((-1.0, 1.0), "arg"), ((float("nan"), 1.0), "arg"),
                      ((fs, float("inf")), "arg"), ((fs, 0.0, 1e3, -1.0), "arg")):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.mix_tone(*bad)
        assert e.value.code == (E_RANGE if code == "range" else E_ARG), (bad, e.value.code)


def test_mix_gain_values_and_refusals():
    assert gpsiq.mix_gain(250.0, MIX_TONE, 0) == 1
    assert gpsiq.mix_gain(250.0, MIX_ROTATED, 10) == 1024
    assert gpsiq.mix_gain(1.0, MIX_STREAM, 8) == 256
    assert gpsiq.mix_gain(-3.5, MIX_STREAM, 1) == -7
    assert gpsiq.mix_gain(1000.0, MIX_TONE, 3) == 32
    assert gpsiq.mix_gain(2.0 ** 31 - 1, MIX_STREAM, 0) == 2 ** 31 - 1
    for bad, code in (((2.0 ** 31, MIX_STREAM, 0), E_RANGE), ((-(2.0 ** 31), MIX_STREAM, 0), E_RANGE), ((1e6, MIX_TONE, 40), E_RANGE),
                      ((1.0, 3, 0), E_ARG), ((1.0, MIX_TONE, -1), E_ARG), ((1.0, MIX_TONE, 41), E_ARG),
                      ((float("nan"), MIX_TONE, 0), E_ARG)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.mix_gain(*bad)
        assert e.value.code == code, (bad, e.value.code)


def test_the_term_is_the_struct_of_the_header():
    text = open(os.path.join(ROOT, "include", "gpsiq_rows.h")).read()
    body = text[text.index("typedef struct gpsiq_mix_term {"):text.index("} gpsiq_mix_term_t;")]
    names = [f[0] for f in gpsiq.MixTerm._fields_]
    at = [body.index(n) for n in ("kind,", "sample_size;", "*src;", "skip;", "gain,", "reserved;", "phase0;", "step;", "rate;", "sweep_period,",
                                  "sweep_offset;", "gate_period,", "gate_on,", "gate_offset,", "reserved2;")]
    assert at == sorted(at) and len(names) == len(at) and C.sizeof(gpsiq.MixTerm) == 80
    assert MIX_MAX_TERMS == 8 and (MIX_STREAM, MIX_ROTATED, MIX_TONE) == (0, 1, 2)
    with pytest.raises(gpsiq.GpsiqError):
        gpsiq.mix_advance([gpsiq.MixTerm.tone(1, 1)] * 9, 1)


# ---- the planner ----------------------------------------------------------------------------------------------------------------------

def test_plans_are_pinned():
    lim = mp.limits()
    assert (lim.threads, lim.max_grid, lim.slot_bytes, lim.max_terms, lim.max_shift) == (256, 4096, 16, 8, 40)
    assert mp.plan(0, 0, SC08) is None
    # the generic kernel: a sample a thread
    assert mp.plan(1, 0, SC08, force=mp.GENERIC) == mp.Plan(0, 1, 256, 0, 1)
    assert mp.plan(257, 0, SC16, 4, force=mp.GENERIC) == mp.Plan(0, 2, 256, 0, 257)
    assert mp.plan(2 ** 31 - 1, 0, SC16, force=mp.GENERIC) == mp.Plan(0, 4096, 256, 0, 2 ** 31 - 1)
    # the row kernel: 16-byte slots, the first one starting `lead` samples before the span
    assert mp.plan(8, 0, SC08, 0, force=mp.ROWS) == mp.Plan(1, 1, 256, 0, 1)
    assert mp.plan(8, 0, SC08, 4, force=mp.ROWS) == mp.Plan(1, 1, 256, 2, 2)
    assert mp.plan(8, 0, SC08, 12, force=mp.ROWS) == mp.Plan(1, 1, 256, 6, 2)
    assert mp.plan(4, 0, SC16, 16, force=mp.ROWS) == mp.Plan(1, 1, 256, 0, 1)
    assert mp.plan(4, 0, SC16, 20, force=mp.ROWS) == mp.Plan(1, 1, 256, 1, 2)
    assert mp.plan(4099, 0, SC16, 8, force=mp.ROWS) == mp.Plan(1, 5, 256, 2, 1026)
    assert mp.plan(2 ** 31 - 1, 2 ** 40, SC08, 0, force=mp.ROWS) == mp.Plan(1, 4096, 256, 0, 2 ** 28)
    # where m or m + offset could wrap inside the span the row kernel does not serve, forced or not
    assert mp.plan(100, 2 ** 63 - 1, SC08, force=mp.ROWS).kernel == 1
    assert mp.plan(100, 2 ** 63, SC08, force=mp.ROWS).kernel == 0
    assert mp.plan(100, 2 ** 64 - 1, SC16, force=mp.AUTO).kernel == 0
    # the default is the measured one (profiles/mix_rates.txt)
    for ss in (SC08, SC16):
        assert mp.plan(10 ** 6, 0, ss).kernel == lim.rows_default


def test_plans_hold_their_invariants_sanitized():
    rng = np.random.default_rng(10)
    req = [("limits",)]
    for _ in range(300):
        nsamp = int(rng.choice([0, 1, 2, 3, 7, 8, 9, 255, 256, 257, 4099, 10 ** 6, 2 ** 31 - 1, int(rng.integers(1, 2 ** 31))]))
        m0 = int(rng.choice([0, 1, 2 ** 32 - 2000, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]))
        req.append(("plan", nsamp, m0, int(rng.choice([1, 2])), 4 * int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 3))))
    for nblocks, nsamp, by, ov in ((0, 100, 400, 0), (7, 100, 400, 0), (7, 100, 400, 2), (7, 100, 400, 100), (1000, 2600000, 10400000, 0),
                                   (5000, 2 ** 30, 2 ** 32, 0), (5000, 2 ** 30, 2 ** 32, 3), (10, 0, 0, 0)):
        req.append(("piece", nblocks, nsamp, by, ov))
    plain, san = mp.ask(req), mp.ask(req, sanitize=True)
    assert plain == san
    assert plain[-8:] == [0, 7, 2, 7, 4, 1, 1, 10]


# ---- gpsiq_runahead --tone: the checks that need no device ---------------------------------------------------------------------------

def runahead(*flags, fs="2600000"):
    exe = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", fs, "2", "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--tone", "1e5"), ("--tone", "1e5,"), ("--tone", "1e5,10,2e5"), ("--tone", "1e5,10,2e5,0"),
                                   ("--tone", "1e5,10,2e5,1e-3,7"), ("--tone", "x,10"), ("--tone", "1e5,10,x"), ("--tone", "1.3e6,10"),
                                   ("--tone", "-1.3e6,10"), ("--tone", "0,10,1.3e6,1e-3"), ("--tone", "0,10,1e5,1e-7"), ("--tone", "0,nan"),
                                   ("--tone", "1e5,10", "--filter", "1e6"), ("--tone", "1e5,10", "--level", "30", "--qmax", "7", "--pack", "4"),
                                   ("--tone", "1,0", "--tone", "2,0", "--tone", "3,0", "--tone", "4,0", "--tone", "5,0")])
def test_runahead_tone_refuses_what_the_stage_cannot_do(flags):
    r = runahead(*flags)
    assert r.returncode == 2 and "usage:" in r.stderr and "--tone" in r.stderr and "--pack 4|2" in r.stderr, (r.returncode, r.stderr)


def test_runahead_tone_accepts_the_rest():
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--tone", "1e5,20"), ("--tone", "-2e5,0,4e5,1e-3", "--cn0", "45"), ("--tone", "1e5,20", "--spectrum", "512"),
                  ("--tone", "1,0", "--tone", "2,0", "--tone", "3,0", "--tone", "4,-3.5", "--level", "30", "--qmax", "100")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
