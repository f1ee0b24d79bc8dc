"""gpsiq_despread on the CPU: the planner (tests/despread_plan.cpp over csrc/gpsiq_despread_plan.h, also built with the address and
undefined-behaviour sanitizers), gpsiq_cn0_estimate against its formula, and the loop closed on the reference alone -- a channel
rendered by the oracle at a set C/N0 (tests/_noise_ref.py's noise) is despread by tests/_despread_ref.py and the estimate comes
back at the set value.  tests/test_gpu_despread.py repeats that case on the device and must match its integers."""
import functools

import numpy as np
import pytest

import _despread_plan as dp
import _despread_ref as dr
import _noise_ref as nr
import _oracle
import gpsiq
from gpsiq.abi import DESPREAD_SUM_DTYPE, SC16


# ---- planner --------------------------------------------------------------------------------------------------------------------

def plans(sanitize=False):
    return dp.query_many([(c.nsamp, c.nblocks, c.seg_len, dp.case_class(c).max_code_step, dp.case_class(c).max_active, c.force, c.target)
                          for c in dp.CASES], sanitize)


def test_every_case_takes_the_kernel_it_is_written_for_and_the_table_reaches_every_instantiation():
    got = plans()
    for c, p in zip(dp.CASES, got):
        assert p is not None and p.kernel == c.kernel, (c.name, p)
        rows = (c.nsamp + 63) // 64
        assert p.threads == 256 and p.grid == p.tiles * c.nblocks and p.tiles * 4 * p.wave_rows >= rows, (c.name, p)
        assert p.seg_rows * 64 == c.seg_len and p.nseg == dr.nseg_of(c.nsamp, c.seg_len), (c.name, p)
        if c.kernel == "generic":
            assert p.wave_rows == 16 and p.tiles == max(1, -(-rows // 64)), (c.name, p)
        else:
            assert p.slots == (4 if p.slots <= 4 else p.slots) and p.slots >= max(a.count("x") for a in c.active) > p.slots - 4, (c.name, p)
    assert sorted({dp.kernel_name(p, c.ss) for c, p in zip(dp.CASES, got)}) == dp.INSTANTIATIONS
    by = {c.name: p for c, p in zip(dp.CASES, got)}
    # the default grid of one 70 001-sample block: five workgroups of one-chunk waves; at a target of one workgroup: runs of 256 rows
    assert (by["seg-2560"].tiles, by["seg-2560"].wave_rows) == (5, 64)
    for name in ("seg-inside-run", "seg-wave-edge", "seg-wg-edge"):
        assert (by[name].tiles, by[name].wave_rows) == (2, 256), by[name]
    p = by["seg-inside-run"]
    assert p.seg_rows % 64 and p.seg_rows < p.wave_rows                        # an edge inside a chunk of a wave's run
    assert by["seg-wave-edge"].seg_rows == by["seg-wave-edge"].wave_rows
    assert by["seg-wg-edge"].seg_rows == 4 * by["seg-wg-edge"].wave_rows and dp.LONG_ROWS > by["seg-wg-edge"].seg_rows


def test_planner_rules():
    cls = dp.pq.SynthClass(int(round(1.023e6 / 2.6e6 * 2 ** 56)), 16, 0)
    # the headline shape: long runs, four workgroups per block
    p = dp.query(260000, 4130, 2560, cls)
    assert (p.kernel, p.slots, p.wave_rows, p.tiles, p.grid, p.nseg) == ("rows", 16, 256, 4, 16520, 102)
    # a whole 2.5 M-sample block in one segment
    p = dp.query(2500000, 1, 1 << 30, cls)
    assert (p.kernel, p.wave_rows, p.nseg) == ("rows", 64, 1) and p.tiles * 256 >= 39063
    # the row kernel's limit is the synthesis row kernel's
    assert dp.query(1000, 1, 64, cls._replace(max_code_step=dp.pq.ROWS_MAX_CODE_STEP)).kernel == "rows"
    assert dp.query(1000, 1, 64, cls._replace(max_code_step=dp.pq.ROWS_MAX_CODE_STEP + 1)).kernel == "generic"
    # nothing to do, or nothing that can be planned
    assert dp.query(1000, 0, 64, cls) is None and dp.query(1000, 1, 100, cls) is None and dp.query(1000, 1, 0, cls) is None
    p = dp.query(0, 3, 64, cls)
    assert p.grid == 3 and p.nseg == 0                                         # the satellites are still reported


def test_planner_under_the_sanitizers():
    """the same table through the program built with -fsanitize=address,undefined: a program of its own"""
    assert plans(sanitize=True) == plans()
    assert dp.query(2147483647, 1, 64, dp.pq.SynthClass(1, 1, 0), sanitize=True).nseg == 33554432


# ---- gpsiq_cn0_estimate ---------------------------------------------------------------------------------------------------------

def sums_of(i, q):
    s = np.zeros(len(i), dtype=DESPREAD_SUM_DTYPE)
    s["i"], s["q"] = i, q
    return s


def test_cn0_estimate_equals_the_formula():
    i = np.array([1000003, 999001, 1002017, 998113, 1000931, 1001477, 997991], dtype=np.int64) * 977
    q = np.array([-1203, 877, 1519, -431, -1777, 263, 1091], dtype=np.int64) * 1013
    for seg_len, fs in ((2560, 2.6e6), (64, 25e6), (26000, 2.6e6)):
        got = gpsiq.cn0_estimate(sums_of(i, q), seg_len, fs)
        m = float(np.mean(i.astype(np.float64)))
        v = (float(((i - m) ** 2).sum()) / 6 + float((q.astype(np.float64) ** 2).sum()) / 7) / 2
        T = seg_len / fs
        cn0 = 10 * np.log10(m * m / (2 * v * T))
        one = 10 / np.log(10) * np.sqrt(1 / 7 + 1 / (7 * T * 10 ** (cn0 / 10)))
        assert got == pytest.approx((cn0, one), rel=1e-12, abs=0)
        assert dr.cn0_estimate(sums_of(i, q), seg_len, fs) == pytest.approx(got, rel=1e-12, abs=0)
    assert gpsiq.cn0_estimate(sums_of(i[:2], q[:2]), 2560, 2.6e6)[1] > 0


@pytest.mark.parametrize("i,q", [([-5, -7, -9], [1, 2, 3]), ([5, -5], [1, 1]), ([0, 0, 0], [4, 4, 4]), ([7, 7, 7], [0, 0, 0]), ([7], [1]), ([], [])])
def test_cn0_estimate_refuses(i, q):
    """a mean that is not positive, no noise at all, fewer than two segments: GPSIQ_E_RANGE"""
    with pytest.raises(gpsiq.GpsiqError) as e:
        gpsiq.cn0_estimate(sums_of(np.array(i, dtype=np.int64), np.array(q, dtype=np.int64)), 2560, 2.6e6)
    assert e.value.code == -2, str(e.value)


def test_the_unit_table_is_what_the_kernels_take_it_for():
    """one table for all channels: the sign enters as half a cycle (entry k + 256 = minus entry k) and entry 511 - k is
    (cos, -sin) of entry k; C^2 + S^2 is 250^2 to within half a percent"""
    s, c = _oracle.load_oracle().tables()
    k = np.arange(512)
    assert np.array_equal(s[(k + 256) % 512], -s) and np.array_equal(c[(k + 256) % 512], -c)
    assert np.array_equal(s[511 - k], -s) and np.array_equal(c[511 - k], c)
    p = (s.astype(np.int64) ** 2 + c.astype(np.int64) ** 2) / 250.0 ** 2 - 1
    assert -0.0044 < p.min() and p.max() < 0.0038 and abs(p.mean()) < 0.0002


# ---- the loop closed on the reference -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loop_reference():
    """(quantised descriptors, noisy int16 stream [nblocks][2 nsamp], sums, prn) of the closed-loop case, computed once"""
    L = dr.LOOP
    orc = _oracle.load_oracle()
    q, _ = gpsiq.quantize_blocks(dr.loop_descriptors(), L["fs"], L["nsamp"])
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    z = nr.noise(L["seed"], sigma, 0, L["nblocks"], L["nsamp"])
    clean = np.stack([orc.block_fixed(q[b], L["nsamp"], SC16) for b in range(L["nblocks"])])
    stream = nr.add_noise16(clean, z)
    sums, prn = dr.despread(orc, q, stream, L["nsamp"], L["seg_len"])
    return q, stream, sums, prn


def test_a_channel_rendered_at_45_dbhz_measures_45_dbhz():
    L = dr.LOOP
    q, stream, sums, prn = loop_reference()
    assert L["nsamp"] % L["seg_len"] == 0 and sums.shape == (L["nblocks"], 2, 26) and np.array_equal(prn, np.tile(np.uint8(L["prn"]), (L["nblocks"], 1)))
    cn0, one = gpsiq.cn0_estimate(sums[:, 0], L["seg_len"], L["fs"])
    print(f"set {L['cn0']} dB-Hz, measured {cn0:.4f} dB-Hz, one sigma {one:.4f} dB over {sums[:, 0].size} segments")
    assert sums[:, 0].size == 1664 and 0.10 < one < 0.12
    assert abs(cn0 - L["cn0"]) <= 4 * one
    # the probe: another satellite at gain 0 adds nothing to the stream and sees the noise floor alone
    pi = sums["i"][:, 1].astype(np.float64).ravel()
    stderr = pi.std(ddof=1) / np.sqrt(pi.size)
    print(f"probe mean {pi.mean():.1f}, standard error {stderr:.1f}")
    assert abs(pi.mean()) <= 4 * stderr
    # both channels see the same floor: v of the probe is what the estimator took for the channel's noise, within its own scatter
    vp = ((pi - pi.mean()) ** 2).sum() / (pi.size - 1)
    sig = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    assert vp == pytest.approx(L["seg_len"] * sig * sig * 250.0 ** 2, rel=4 * np.sqrt(2.0 / pi.size) + 0.005)
