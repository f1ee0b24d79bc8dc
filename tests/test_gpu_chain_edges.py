"""The device carrier chain (csrc/gpsiq_chain_kernels.hip: chain_prepare, chain_lanes<4|8|16|32>) at the edges of its scans and
workgroups, with its maps audited over their whole range (tests/_chain_audit.py; tests/test_chain_audit.py does the same to the host
twin, on the CPU).  Every case checks four things:
  1. audit      every device map with ok != 0 tried at lo, hi, next to them, per parity and in between, against the reference's
                accumulator started there (walk() up to 4 096 samples, serial_end() beyond);
  2. chain      gpsiq.chain_link with the device maps == gpsiq.reference_chain, bit for bit;
  3. link rate  the check that sees through the fallback: a wrong carry or a wrong neighbour addend only costs walked blocks, so for
                every active block the device map admits the TRUE start state exactly where the host twin's does -- at most 1 block
                in 1 000 may differ (the two sum the drift in another order: an estimate on a knife edge), none on an
                engineered-event block or the block after it, where the two records also agree on ok and on why;
  4. end        the estimator state handed on == the host's (phase, satellite, f_carr exactly, drift to rounding; carr 0, EXACT never,
                RESEEDED by the documented rule).
A timeline is built 16 slots wide and run in column groups of the case's nchan (slots are independent), so that the kernels' slot
index blockIdx / groups is exercised with 1, 5 and 16 channels.

The lanes walk |c| < 2^-6 only (FpWalk::setup_head), so a block of 32 stretches (128 cycles) has more than 8 192 samples: the lane and
tie groups use 9 600 (reference: serial_end); the scan groups, whose work is along the block axis, 600 (reference: walk).
What a single small case cannot reach (ok = 1, maps of 32 stretches, ...) is asserted over the file, in the last test."""
import numpy as np
import pytest

import gpsiq
import _chain_audit as A
from gpsiq.abi import CHAIN_EST_DTYPE, CHAIN_EXACT
from test_chain_parallel import timeline

pytestmark = pytest.mark.gpu
K_WHY_PREV = 2              # gpsiq_lane.h kWhyPrev
TOTAL = {}                  # group -> [Audit, blocks whose admission differed, active blocks]


@pytest.fixture(scope="module")
def ctx():
    c = gpsiq.Context(0)
    yield c
    c.close()


def check(ctx, group, cin16, record16, fs, nsamp, ms, nchan, start16=None, carr_in16=None, prn_in16=None, seed=0):
    tot = TOTAL.setdefault(group, [A.Audit(), 0, 0])
    out = []
    for s0 in range(0, cin16.shape[1], nchan):
        cols = slice(s0, min(s0 + nchan, cin16.shape[1]))
        cin = np.ascontiguousarray(cin16[:, cols])
        record = [dict(e, slot=e["slot"] - s0) for e in record16 if cols.start <= e["slot"] < cols.stop]
        start = None if start16 is None else np.ascontiguousarray(start16[cols])
        carr_in = None if carr_in16 is None else carr_in16[cols]
        prn_in = None if prn_in16 is None else prn_in16[cols]
        want = gpsiq.reference_chain(cin, fs, nsamp, carr_in, prn_in)
        maps, end, _ = gpsiq.chain_maps(cin, fs, nsamp, start=start, max_stretches=ms, ctx=ctx)
        hmaps, hend = gpsiq.chain_maps(cin, fs, nsamp, start=start, max_stretches=ms)
        # 1. the audit
        res = A.audit(cin, maps, fs, nsamp, np.random.default_rng(seed + s0), 2, ms)
        res.assert_caps()
        # 2. the chain
        got = gpsiq.chain_link(cin, maps, fs, nsamp, carr_in, prn_in)
        for g, w, what in zip(got, want, ("carr_start", "carr_end", "last_prn")):
            assert g.tobytes() == w.tobytes(), what
        # 3. the link rate
        act = cin["prn"] > 0
        adm_d, adm_h = A.true_admission(maps, cin, want[0]), A.true_admission(hmaps, cin, want[0])
        differ = adm_d != adm_h
        ev = A.event_blocks(record, cin.shape) & act
        say = [(int(b), int(s), hex(int(maps["info"][b, s])), hex(int(hmaps["info"][b, s])), float(maps["xs"][b, s]).hex(), float(hmaps["xs"][b, s]).hex(),
                float(want[0][b, s]).hex()) for b, s in np.argwhere(differ)[:8]]
        print(f"{group} nb {cin.shape[0]} slots {cols.start}..{cols.stop - 1} ms {ms}: {res}; admission differs on {int(differ.sum())} of {int(act.sum())}"
              + (f" (block, slot, device info, host info, device xs, host xs, true start): {say}" if say else ""))
        assert not (differ & ev).any(), say
        assert int(differ.sum()) * 1000 <= int(act.sum()), say
        same_why = (maps["info"] == hmaps["info"]) | ((hmaps["info"] == 0) & ((maps["info"] >> 8) == K_WHY_PREV))
        wrong = ev & ((maps["ok"] != hmaps["ok"]) | ~same_why)
        assert not wrong.any(), [(int(b), int(s), maps[b, s], hmaps[b, s]) for b, s in np.argwhere(wrong)[:4]]
        good = maps["ok"] != 0
        why, _, _ = A.link(maps[good], want[0][good])
        assert not np.any(why == 2), "a true start that is no whole number of units off its representative"
        assert np.all(np.abs(want[0][good] - maps["xs"][good]) < 1e-9)
        # 4. the estimator state handed on
        for f in ("r_hi", "r_lo", "prn", "f_carr"):
            assert np.array_equal(end[f], hend[f]), (f, end[f], hend[f])
        assert np.allclose(end["drift"], hend["drift"], rtol=1e-6, atol=1e-18)
        assert np.all(end["carr"] == 0.0) and not np.any(end["flags"] & CHAIN_EXACT)
        assert np.array_equal(end["flags"], A.expected_device_flags(hend, start, cin)), (end["flags"], hend["flags"])
        tot[0] += res
        tot[1] += int(differ.sum())
        tot[2] += int(act.sum())
        out.append((maps, end, got, adm_d, adm_h))
    return out


# ---- chain_prepare's scan edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,nchan", list(zip(A.SCAN_BLOCKS, (1, 5, 16, 1, 5, 16, 5, 1, 16))))
def test_scan_edges(ctx, nb, nchan):
    cin, record = A.scan_edge_timeline(nb)
    check(ctx, "scan", cin, record, A.FS, 600, 32, nchan, seed=nb)


@pytest.mark.parametrize("nsamp,nchan", [(33333, 5), (260000, 16)])
def test_long_blocks(ctx, nsamp, nchan):
    """Doppler inside +-6 kHz, blocks of the lengths of the other chain tests: serial_end is the reference"""
    cin = timeline(nsamp % 97, 130, 16)
    check(ctx, "long", cin, [], A.FS, nsamp, 32, nchan, seed=nsamp)


# ---- continuation through `start` ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut,nchan", [(1, 16), (64, 5), (1024, 1), (1025, 16)])
@pytest.mark.parametrize("how", ["estimate", "exact", "no_satellite", "other_satellite"])
def test_a_timeline_continued_through_start(ctx, cut, nchan, how):
    """cut at 1 / 64 / 1024 / 1025 blocks and continued from the device's own `end` (an estimate: block 0 links from c_before, the
    tail of a block that is not in this launch), from the exact accumulator, from a state with prn = 0, and from an exact state
    of another satellite than block 0's"""
    fs, nsamp = A.FS, 600
    cin, record = A.scan_edge_timeline(cut + 70)
    key = ("head", cut)
    if key not in TOTAL:
        m0, est, _ = gpsiq.chain_maps(cin[:cut], fs, nsamp, max_stretches=32, ctx=ctx)
        TOTAL[key] = (est, gpsiq.chain_link(cin[:cut], m0, fs, nsamp))
    est, (s0, e0, p0) = TOTAL[key]
    assert s0.tobytes() == gpsiq.reference_chain(cin[:cut], fs, nsamp)[0].tobytes()
    start = est.copy()
    prn_in = p0.copy()
    if how != "estimate":
        start = np.zeros(A.NC, dtype=CHAIN_EST_DTYPE)
        start["carr"], start["prn"], start["flags"], start["f_carr"] = e0, p0, CHAIN_EXACT, cin["f_carr"][cut - 1]
        if how == "no_satellite":
            prn_in = np.zeros_like(p0)
        elif how == "other_satellite":
            prn_in = np.where(cin["prn"][cut] > 0, 1 + cin["prn"][cut] % 32, 1).astype(np.int32)
        start["prn"] = prn_in
    tail = [dict(e, block=e["block"] - cut) for e in record if e["block"] >= cut]
    res = check(ctx, "continued", cin[cut:], tail, fs, nsamp, 32, nchan, start16=start, carr_in16=e0, prn_in16=prn_in, seed=cut)
    if how in ("estimate", "exact"):                                  # the whole timeline is the serial chain's
        starts = np.concatenate([s0, np.concatenate([r[2][0] for r in res], axis=1)])
        assert starts.tobytes() == gpsiq.reference_chain(cin, fs, nsamp)[0].tobytes()
    if how == "estimate":                                             # block 0 of the ordinary slots links, from an estimate
        adm0 = np.concatenate([r[3][0] for r in res])
        assert adm0[11:].sum() >= 4 and not np.any(start["flags"] & CHAIN_EXACT), adm0


# ---- chain_lanes' workgroup and lane edges -----------------------------------------------------------------------------------------
LANE_CASES = [(kseg, ms, nb) for kseg, mss in A.LANE_SEGS.items() for ms in mss for nb in A.lane_blocks(kseg)]


@pytest.mark.parametrize("kseg,ms,nb", LANE_CASES)
def test_lane_edges(ctx, kseg, ms, nb):
    assert A.lanes_per_block(ms) == kseg
    cin, record = A.lane_edge_timeline(kseg, nb)
    nchan = (1, 5, 16)[LANE_CASES.index((kseg, ms, nb)) % 3]
    check(ctx, "lanes", cin, record, A.FS, A.NS_LANES, ms, nchan, seed=nb + ms)


@pytest.mark.parametrize("nsamp", [1, 7])
def test_blocks_of_a_few_samples(ctx, nsamp):
    cin, record = A.lane_edge_timeline(32, 25, nsamp=nsamp)
    check(ctx, "few", cin, record, A.FS, nsamp, 32, 16, seed=nsamp)


# ---- exact ties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [1, 4, 8, 16, 32])
@pytest.mark.parametrize("nsamp", [4096, A.NS_LANES])
def test_exact_ties(ctx, nsamp, ms):
    cin, record = A.tie_timeline(40, nsamp)
    check(ctx, "ties", cin, record, A.FS_TIE, nsamp, ms, (16, 5)[ms % 2], seed=ms)


def test_what_the_file_reached():
    """over all cases above (run the whole file): the population conditions of tests/test_chain_audit.py on the DEVICE's maps.
    ok = 2 never comes out of the join (tests/test_chain_audit.py says why)."""
    groups = ("scan", "long", "continued", "lanes", "few", "ties")
    assert all(g in TOTAL for g in groups), "run the whole file"
    for g in groups:
        print(f"{g}: {TOTAL[g][0]}; device / host admission differed on {TOTAL[g][1]} of {TOTAL[g][2]} active blocks")
    tot = sum((TOTAL[g][0] for g in groups), A.Audit())
    assert tot.ok1 > 100 and tot.ok3 > 1000 and tot.cum_differ > 100, tot
    assert tot.grid1 > 1000 and tot.grid2 > 1000 and tot.c_pos > 1000 and tot.c_neg > 1000 and {1, 32} <= tot.seg, tot
    ties = TOTAL["ties"][0]
    assert ties.ok1 > 0 and ties.cum_differ > 100 and ties.odd_at_lo > 100 and ties.odd_at_hi > 100, ties
    assert {1, 2, 4, 5, 8, 9, 16, 17, 31, 32} <= TOTAL["lanes"][0].seg, TOTAL["lanes"][0]
