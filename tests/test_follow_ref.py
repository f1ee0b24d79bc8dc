"""gpsiq_follow on the CPU: the numpy restatement (tests/_follow_ref.py) held against a second, scalar statement of the contract and
against an epoch computed by hand; gpsiq_follow_gains and gpsiq_follow_bits against their formulas, with their argument and range
errors; the planner (tests/follow_plan.cpp over csrc/gpsiq_follow_plan.h, also built with the address and undefined-behaviour
sanitizers); the claims of the GPU case table; and the design itself: the restatement, started a fifth of a chip and 120 Hz off,
locks onto a stream rendered by the oracle's closed form and reads back every data bit.  tests/test_gpu_follow.py holds the kernel to
the restatement, tests/test_gpu_follow_signal.py repeats the lock on the device."""
import numpy as np
import pytest

import _follow_plan as fp
import _follow_ref as fr
import _oracle
import gpsiq
from gpsiq.abi import FOLLOW_CFG_DTYPE, FOLLOW_EPOCH_DTYPE, FOLLOW_STATE_DTYPE, SC08, SC16


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def test_an_epoch_of_the_code_itself_computed_by_hand(orc):
    """PRN 5 at one chip and a quarter of a cycle per sample, I = ca cos, Q = ca sin (the stream of tests/test_acquire_ref.py's first
    case, a whole period of it): yi = 62 504 ca, yq = 0, so the prompt sum is 1023 * 62 504 = 63 941 592; the early and late replicas,
    half a chip off, read the same chip as the prompt (spacing 2^55, fraction 0 resp. 2^55) or its neighbour: early at fraction 0 is
    the prompt's chip, late the chip before, whose sum is 62 504 times the code's autocorrelation at one chip, -1.
    The second epoch does not fit: status 1 after one record, and the state has moved one period on."""
    s, c = orc.tables()
    chips = orc.codegen(5).astype(np.int64)
    ca = 1 - 2 * chips
    idx = 128 * (np.arange(1023) % 4)
    stream = np.stack([ca * c[idx], ca * s[idx]], axis=1).astype(np.int16).ravel()
    st = fr.make_state(5, code_step=1 << 56, carr_step=1 << 57)
    rec, n, out = fr.follow(orc, stream, fr.make_cfg(), [st], 4)
    assert n[0] == 1 and out[0]["status"] == fr.SPAN_END
    r = rec[0, 0]
    assert (int(r["nsamp"]), int(r["ip"]), int(r["qp"])) == (1023, 63941592, 0)
    assert (int(r["ie"]), int(r["qe"])) == (63941592, 0) and (int(r["il"]), int(r["ql"])) == (-62504, 0)
    o = out[0]
    assert (int(o["sample"]), int(o["chip"]), int(o["code_frac"]), int(o["epoch"]), int(o["have_prev"])) == (1023, 0, 0, 1, 1)
    assert int(o["carr_phase"]) == (1023 << 57) % (1 << 59)
    # the scaled prompt: 63 941 592 has 26 bits, so four are shifted out
    assert (int(o["prev_ip"]), int(o["prev_qp"])) == (63941592 >> 4, 0)


@pytest.mark.parametrize("name", ["mixed-int16", "lengths-int8", "spacing-chip", "spacing-one", "late-wrap", "carrier", "range-code", "zero-int8", "min-int16"])
def test_the_vectorised_restatement_equals_the_scalar_one(orc, name):
    """the first epochs of cases of the GPU table (all of them where the case is short), every satellite: records and final state"""
    case = [c for c in fp.CASES if c.name == name][0]
    stream, cfg, states, _ = fr.materialise(orc, case, fp.CASES.index(case))
    few = 3
    short = stream[:2 * min(len(stream) // 2, 2400)]
    rec, n, out = fr.follow(orc, short, cfg, states, few)
    for p in range(len(states)):
        records, st = fr.follow_scalar(orc, short, cfg, states[p], few)
        assert len(records) == n[p]
        for k, r in enumerate(records):
            assert fr.record_tuple(rec[p, k]) == r, (p, k)
        for f in FOLLOW_STATE_DTYPE.names:
            if f != "reserved":
                assert int(out[p][f]) == (st[f] % (1 << 64) if f == "code_step" else st[f]), (p, f)


def test_the_split_product_of_the_tap_chips_is_the_full_one():
    """_tap_chips at the corners of its domain against Python integers: the largest base, step and sample index"""
    n = np.array([0, 1, 2, 511, 1023, 2599, 16367], dtype=np.uint64)
    for base in (0, 1, (1 << 56) - 1, 1 << 56, fr.PERIOD - 1, fr.PERIOD + (1 << 56)):
        for c in (1 << 52, (1 << 52) + 1, 3 << 55, (1 << 57) - 1, 0x1777777777777f):
            want = [((base + int(k) * c) >> 56) % 1023 for k in n]
            assert list(fr._tap_chips(base, c, n)) == want, (base, c)


def test_the_case_table_is_what_its_names_say(orc):
    """every claim of tests/_follow_plan.py's table holds on the restatement: the pinned statuses; first epochs of 128, 129, 127, 65
    and 64 samples; epochs of 512 and of 16368 samples at the ends of the code step's range; an epoch of one sample; the carrier
    wrapping 2^59 hundreds of times within an epoch; both loops entered where the table says mid-run; a status 3 beside satellites that
    run to the end of the span; an all-zero stream that moves nothing"""
    by = {}
    for i, c in enumerate(fp.CASES):
        by[c.name] = (c,) + fr.materialise(orc, c, i)
        ref = by[c.name][4]
        if c.expect is not None:
            assert tuple(int(s) for s in ref[2]["status"]) == c.expect, c.name
        assert all(s != fr.RUNNING for s in ref[2]["status"]) and len({c.name for c in fp.CASES}) == len(fp.CASES)
    first = lambda name: [int(v) for v in by[name][4][0][:, 0]["nsamp"]]
    assert first("lengths") == first("lengths-int8") == [128, 129, 127, 65, 64]
    assert first("step-max")[0] == 512 and first("step-min") == [16368, 8176] and first("mixed-int16")[2] == 1
    assert {c.ss for c in fp.CASES} == {SC08, SC16} and {c.base for c in fp.CASES} >= {0, 4, 12}
    rec = by["carrier"][4][0]
    assert all(abs(int(r["carr_step"])) * int(r["nsamp"]) >> 59 > 100 for r in rec[:, 0]) and int(rec[0, 0]["carr_step"]) < 0
    c, _, _, _, ref = by["mixed-int16"]
    assert c.cfg["pull_epochs"] == 10 and min(ref[1]) > 20
    assert max(by["pull-always"][4][1]) < by["pull-always"][0].cfg["pull_epochs"] and by["pull-never"][0].cfg["pull_epochs"] == 0
    st = by["range-carrier"][4][2]["status"]
    assert fr.RANGE in st and st[2] == fr.SPAN_END
    z = by["zero-int16"][4]
    assert all(int(z[0][f].max()) == 0 and int(z[0][f].min()) == 0 for f in fr.SUMS)
    late = by["late-wrap"][0].states
    assert all(s.get("chip", 0) == 0 and s["code_frac"] < by["late-wrap"][0].cfg.get("spacing", 1 << 55) for s in late)
    # a cut case ends on its record's last sample
    cut = by["exact-end"]
    assert len(cut[1]) // 2 == int(cut[4][0][0, 11]["sample"]) + int(cut[4][0][0, 11]["nsamp"])


def test_following_in_pieces_gives_the_records_of_one_call(orc):
    """the restatement's own continuation property (the GPU test asks the same of the device): 13 epochs, then from the returned state"""
    case = fp.CASES[0]
    stream, cfg, states, ref = fr.materialise(orc, case, 0)
    a = fr.follow(orc, stream, cfg, states, 13)
    assert list(a[1]) == [13] * len(states) and all(s == fr.FULL for s in a[2]["status"])
    b = fr.follow(orc, stream, cfg, a[2], case.max_epochs)
    for p in range(len(states)):
        whole = np.concatenate([a[0][p, :13], b[0][p, :b[1][p]]])
        assert whole.tobytes() == ref[0][p, :ref[1][p]].tobytes()
    assert b[2].tobytes() == ref[2].tobytes()


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args", [(2.6e6, 0.25, 18.0, 5.0), (2.6e6, 0.05, 25.0, 3.0), (4.0e6, 0.25, 18.0, 5.0), (1.0e6, 0.5, 40.0, 1.0)])
def test_gains_against_the_formulas(args):
    cfg = gpsiq.follow_gains(*args)
    assert cfg.dtype == FOLLOW_CFG_DTYPE and cfg.shape == (1,)
    want = fr.gains(*args)
    assert {f: int(cfg[0][f]) for f in want} == want and int(cfg[0]["reserved"]) == 0
    assert int(cfg[0]["spacing"]) == 1 << 55 and int(cfg[0]["pull_epochs"]) == 100


def test_gains_errors():
    for bad in [(0.0, 0.25, 18, 5), (-1.0, 0.25, 18, 5), (float("inf"), 0.25, 18, 5), (float("nan"), 0.25, 18, 5), (2.6e6, 0.25, 0.0, 5), (2.6e6, 0.25, 18, -5.0),
                (2.6e6, 0.25, float("nan"), 5), (2.6e6, 0.0, 18, 5)]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.follow_gains(*bad)
        assert e.value.code == -1, bad
    # a gain that leaves [0, 2^46): GPSIQ_E_RANGE
    for bad in [(10.0, 0.25, 18, 5), (2.6e6, 1e9, 18, 5), (2.6e6, 0.25, 18, 1e12)]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.follow_gains(*bad)
        assert e.value.code == -2, bad


def records_of(ip):
    e = np.zeros(len(ip), dtype=FOLLOW_EPOCH_DTYPE)
    e["ip"] = ip
    e["qp"] = 7                                     # never read
    return e


def test_bits_against_the_restatement():
    rng = np.random.default_rng(5)
    for n, skip in [(40, 0), (41, 1), (59, 0), (60, 0), (333, 17), (800, 250), (45, 5)]:
        ip = rng.integers(-2 ** 38, 2 ** 38, size=n)
        off, bits = gpsiq.follow_bits(records_of(ip), skip)
        want = fr.bits(ip, skip)
        assert off == want[0] and bits.dtype == np.int8 and np.array_equal(bits, want[1]), (n, skip)
    # a real bit pattern whose edge is 7 epochs in: the offset is found and the bits come out
    data = np.array([1, -1, -1, 1, 1, 1, -1, 1, -1, -1])
    ip = np.concatenate([np.full(7, -5000), np.repeat(data, 20) * 5000, np.full(9, 5000)]) + rng.integers(-300, 300, size=216)
    off, bits = gpsiq.follow_bits(records_of(ip), 0)
    assert off == 7 and np.array_equal(bits, data)


def test_bits_ties_zero_sums_and_too_few_epochs():
    # every offset equal: the lowest wins, and a constant stream has one sign
    off, bits = gpsiq.follow_bits(records_of(np.full(100, 3)), 0)
    assert off == 0 and np.array_equal(bits, np.ones(5, dtype=np.int8))
    # a square wave of period 20: offsets 0 and 10 are the worst (every group sums to zero), 5 and 15 tie for the best and 5 wins
    ip = np.tile(np.concatenate([np.full(10, 4), np.full(10, -4)]), 4)
    off, bits = gpsiq.follow_bits(records_of(ip), 0)
    want = fr.bits(ip, 0)
    assert (off, list(bits)) == (want[0], list(want[1])) and off == 0 and list(bits) == [0, 0, 0, 0]
    # a group that sums to zero is bit 0; all zeros: offset 0 and every bit 0
    ip = np.concatenate([np.full(20, 9), np.tile([6, -6], 10), np.full(20, -9)])
    off, bits = gpsiq.follow_bits(records_of(ip), 0)
    assert off == 0 and list(bits) == [1, 0, -1]
    off, bits = gpsiq.follow_bits(records_of(np.zeros(64, dtype=np.int64)), 3)
    assert off == 0 and list(bits) == [0, 0, 0]
    # fewer than 40 epochs after skip: GPSIQ_E_RANGE; a negative skip: GPSIQ_E_ARG
    for n, skip in [(39, 0), (45, 6), (0, 0), (40, 100)]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            gpsiq.follow_bits(records_of(np.ones(n, dtype=np.int64)), skip)
        assert e.value.code == -2 and fr.bits(np.ones(n), skip) is None
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.follow_bits(records_of(np.ones(50, dtype=np.int64)), -1)
    assert e.value.code == -1


def test_follow_start_fills_the_state_the_header_states():
    steps = gpsiq.acquire_steps(2.6e6, -5000.0, 250.0)
    st = gpsiq.follow_start([7, 19], [1234, 5], [3, 40], *steps)
    assert st.dtype == FOLLOW_STATE_DTYPE and st.shape == (2,)
    for k, (prn, s, d) in enumerate([(7, 1234, 3), (19, 5, 40)]):
        want = fr.make_state(prn, sample=s, code_step=steps[0], carr_step=steps[1] + d * steps[2])
        assert st[k].tobytes() == want.tobytes()
    assert int(st[0]["carr_int"]) == int(st[0]["carr_step"]) == steps[1] + 3 * steps[2] and int(st[0]["have_prev"]) == 0


# ---- gpsiq_runahead --follow: the checks that need no device ------------------------------------------------------------------------

def test_runahead_follow_argument_checks():
    """--follow takes a time in (0, 10] seconds and needs --acquire; a well-formed line gets past the checks and stops at the RINEX
    file that is not there"""
    from test_acquire_ref import runahead
    for flags in (("--follow", "0.6"), ("--acquire", "--follow", "0"), ("--acquire", "--follow", "-1"), ("--follow", "10.5", "--acquire"),
                  ("--acquire", "--follow", "nan"), ("--cn0", "55", "--follow", "0.6", "--level", "42")):
        r = runahead(*flags)
        assert r.returncode == 2 and "usage:" in r.stderr and "--follow" in r.stderr, (flags, r.returncode, r.stderr)
    for flags in (("--acquire", "--follow", "0.6"), ("--follow", "0.6", "--acquire"), ("--cn0", "55", "--level", "42", "--acquire", "--follow", "10")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)


# ---- the planner --------------------------------------------------------------------------------------------------------------------

def test_the_planner_under_the_sanitizers():
    """every request of the GPU table and the corners of the argument ranges, through the program built with ASan and UBSan: the same
    answers as the plain build, and every plan holds its own invariants (the program exits non-zero otherwise)"""
    top = 2 ** 31 - 1
    reqs = [(c.nsamp, c.ss, len(c.states), c.max_epochs, k, r) for c in fp.CASES for k in (None, 7) for r in (0, 6, 7, c.max_epochs)]
    reqs += [(top, 1, 32, (1 << 30) // 96 // 32, None, 4096), (top, 2, 1, (1 << 30) // 96, 1, 100), (0, 1, 1, 1, None, 0), (5, 2, 3, 100, None, 5),
             (100, 1, 1, 1, 4096, 1), (100, 1, 1, 1, 4097, 1), (100, 1, 1, 1, -3, 1), (10 ** 7, 2, 32, 8192, None, 8192), (10 ** 7, 2, 32, 8192, 4096, 4095)]
    nothing = [(100, 3, 1, 1, None, 0), (100, 0, 1, 1, None, 0), (-1, 1, 1, 1, None, 0), (100, 1, 0, 1, None, 0), (100, 1, 33, 1, None, 0), (100, 1, 1, 0, None, 0),
               (top + 1, 1, 1, 1, None, 0), (100, 1, 32, (1 << 30) // 96 // 32 + 1, None, 0), (100, 1, 1, top + 1, None, 0)]
    plain, checked = fp.query_many(reqs + nothing), fp.query_many(reqs + nothing, sanitize=True)
    assert plain == checked
    assert all(p is not None for p in plain[:len(reqs)]) and all(p is None for p in plain[len(reqs):])
    for r, p in zip(reqs, plain):
        knob = r[4] if r[4] is not None and 1 <= r[4] <= fp.PER_LAUNCH else fp.PER_LAUNCH
        assert p.grid == r[2] and p.threads == 256 and p.per_launch == knob and p.records == r[2] * r[3] and p.record_bytes == 96 * p.records
        assert p.launches == r[5] // knob + 1 and p.max_launches == min(r[3], r[0]) // knob + 1


# ---- the design: the restatement locks onto a rendered stream ---------------------------------------------------------------------

def test_the_loop_locks_onto_a_stream_of_the_oracle_s_closed_form(orc):
    """One satellite of the signal scenario (tests/_follow_signal.py), rendered noiseless in int16 by the oracle's closed form; the
    restatement starts at the sample nearest the code's period start (up to a fifth of a chip off) and 120 Hz off, as the peak of a
    search with 250 Hz bins may be, and must meet the GPU signal test's own conditions from epoch 250 on: code within a quarter chip,
    no carrier cycle slipped, and every data bit read back in one polarity."""
    import _follow_signal as fs_
    sc = fs_.scenario(orc, nchan=1)
    stream = np.concatenate([orc.block_fixed(sc.q[b], sc.nsamp, SC16) for b in range(sc.nblocks)])
    start = fs_.truth_start(sc, 0, freq_error_hz=120.0)
    rec, n, out = fr.follow(orc, stream, gpsiq.follow_gains(sc.fs, 0.25, 18.0, 5.0), [start], 900)
    assert out[0]["status"] == fr.SPAN_END and n[0] > 700
    fs_.assert_locked(sc, 0, rec[0, :n[0]])
