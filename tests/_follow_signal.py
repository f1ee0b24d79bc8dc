"""The signal scenario of the follower's tests (tests/test_follow_ref.py on the CPU, tests/test_gpu_follow_signal.py on the device):
eight 0.1 s blocks at 2.6 Msps of channels whose code, data bits and carrier run on from block to block, and the lock conditions of
the issue as assertions on a satellite's records.  Truth is the quantised descriptors through the closed form of include/gpsiq.h
(tests/_follow_ref.py: truth_code_phase, truth_data_bit), never the follower.  TEST INFRASTRUCTURE."""
import collections

import numpy as np

import _follow_ref as fr
from gpsiq.scenario import synth_blocks

Scenario = collections.namedtuple("Scenario", "fs nsamp nblocks desc q")
FS, NSAMP, NBLOCKS = 2.6e6, 260000, 8
LOCKED_FROM = 250                       # the epoch from which the conditions hold


def descriptors(nchan, nblocks=NBLOCKS, seed=20251, doppler_hz=4000.0):
    """CHAN_DTYPE [nblocks][nchan]: block 0 from the synthetic scenario helper (every gain 1.0, so that one noise level is one C/N0),
    every later block where the block before it ends: code phase, code period, bit and word counters stepped by a block's samples, the
    Doppler constant.  (The carrier phase is carried by the quantiser.)"""
    d0 = synth_blocks(1, nchan, seed=seed, doppler_hz=doppler_hz, prn0=3)[0]
    d = np.zeros((nblocks, nchan), dtype=d0.dtype)
    for c in range(nchan):
        e = d0[c].copy()
        e["gain"] = 1.0
        e["iword"] = int(e["iword"]) % 40                 # the eight blocks stay inside the sixty words
        for b in range(nblocks):
            d[b, c] = e
            total = float(e["code_phase"]) + NSAMP * float(e["f_code"]) / FS
            periods = int(np.floor(total / 1023.0))
            e["code_phase"] = total - 1023.0 * periods
            icode = int(e["icode"]) + periods
            ibit = int(e["ibit"]) + icode // 20
            e["icode"], e["ibit"], e["iword"] = icode % 20, ibit % 30, int(e["iword"]) + ibit // 30
    return d


def scenario(orc, nchan=4):
    d = descriptors(nchan)
    return Scenario(FS, NSAMP, NBLOCKS, d, orc.quantize_blocks(d, FS, NSAMP))


def code_phase_at(sc, ch, m):
    return fr.truth_code_phase(sc.q[m // sc.nsamp, ch], m % sc.nsamp)


def data_sign_at(sc, ch, m):
    """+1 / -1: the sign the channel is rendered with under sample m, the code apart"""
    return 1 - 2 * fr.truth_data_bit(sc.q[m // sc.nsamp, ch], m % sc.nsamp)


def carrier_advance(sc, ch, m0, m1):
    """the descriptors' carrier advance over samples [m0, m1), an exact integer in units of 2^-59 cycle"""
    adv = 0
    for b in range(sc.nblocks):
        lo, hi = max(m0, b * sc.nsamp), min(m1, (b + 1) * sc.nsamp)
        if hi > lo:
            adv += (hi - lo) * int(sc.q[b, ch]["carr_step"])
    return adv


def truth_start(sc, ch, freq_error_hz=0.0, sample_error=0):
    """the state an acquisition peak gives: the sample nearest the first start of a code period, the nominal code step, and a
    carrier step freq_error_hz off the channel's"""
    q0 = sc.q[0, ch]
    phase0 = int(q0["chip0"]) + int(q0["code_frac"]) / 2.0 ** 56
    s = int(np.rint((1023.0 - phase0) * 2.0 ** 56 / int(q0["code_step"]))) + sample_error
    return fr.make_state(int(q0["prn"]), sample=s, code_step=int(np.rint(1.023e6 / sc.fs * 2.0 ** 56)),
                         carr_step=int(np.rint((float(sc.desc[0, ch]["f_carr"]) + freq_error_hz) / sc.fs * 2.0 ** 59)))


def code_errors(sc, ch, rec):
    """chips, in [-511.5, 511.5): the records' code phase less the descriptors' at the same sample"""
    return np.array([((int(r["chip"]) + int(r["code_frac"]) / 2.0 ** 56 - code_phase_at(sc, ch, int(r["sample"])) + 511.5) % 1023.0) - 511.5 for r in rec])


def assert_code_locked(sc, ch, rec):
    err = code_errors(sc, ch, rec[LOCKED_FROM:])
    assert len(err) > 400 and np.abs(err).max() < 0.25, (ch, float(np.abs(err).max()))


def assert_carrier_never_slipped(sc, ch, rec):
    tail = rec[LOCKED_FROM:]
    mine = sum(int(r["nsamp"]) * int(r["carr_step"]) for r in tail)
    m0, m1 = int(tail[0]["sample"]), int(tail[-1]["sample"]) + int(tail[-1]["nsamp"])
    assert abs(mine - carrier_advance(sc, ch, m0, m1)) < 1 << 58, (ch, (mine - carrier_advance(sc, ch, m0, m1)) / 2.0 ** 59)


def assert_bits_read(sc, ch, rec, follow_bits):
    """follow_bits (the library's): every bit from LOCKED_FROM on equals the descriptors' data bit of those twenty code periods, in one
    polarity; and the twenty periods of a group do carry one bit"""
    off, bits = follow_bits(rec, LOCKED_FROM)
    assert len(bits) == (len(rec) - LOCKED_FROM - off) // 20 and len(bits) >= 20
    want = []
    for j in range(len(bits)):
        group = rec[LOCKED_FROM + off + 20 * j:LOCKED_FROM + off + 20 * j + 20]
        signs = {data_sign_at(sc, ch, int(r["sample"]) + int(r["nsamp"]) // 2) for r in group}
        assert len(signs) == 1, (ch, j, "the group straddles a bit edge")
        want.append(signs.pop())
    want = np.array(want, dtype=np.int8)
    assert len(set(want)) == 2, "the scenario's bits do not change: nothing would be shown"
    assert np.array_equal(bits, want) or np.array_equal(bits, -want), (ch, int((bits == want).sum()), int((bits == -want).sum()), len(bits))


def assert_locked(sc, ch, rec, follow_bits=None):
    import gpsiq
    assert_code_locked(sc, ch, rec)
    assert_carrier_never_slipped(sc, ch, rec)
    assert_bits_read(sc, ch, rec, follow_bits or gpsiq.follow_bits)
