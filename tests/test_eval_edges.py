"""tests/_eval_edges.py held to what it claims, on the CPU: the timelines of tests/test_gpu_eval_edges.py really have an event of
every kind on and next to every boundary (recomputed from prn and f_carr alone), the Doppler-through-zero slots really break the
certified map at their boundary, and the two references are those of the parts of the suite that are already trusted: the
independent walker float_reference == the library's serial chain (gpsiq.reference_chain) bit for bit and == the reference's own
loop (oracle/_ref), fixed_reference == the oracle's sequential form."""
import numpy as np
import pytest

import _eval_edges as ee
import gpsiq
from gpsiq.abi import SC08, SC16, SINK_IQFILE

FS = ee.FS


def seeds_and_unused(d):
    """from prn alone: where a slot is unused, and where it seeds (block 0, or another satellite than the block before)"""
    prn = np.maximum(d["prn"].astype(np.int64), 0)
    unused = prn == 0
    seeds = ~unused
    seeds[1:] &= prn[1:] != prn[:-1]
    return prn, unused, seeds


def check_event(d, e):
    """the descriptors agree with one claimed event"""
    prn, unused, seeds = seeds_and_unused(d)
    nb = d.shape[0]
    kind, s = e["key"][0], e["slot"]
    if kind in ("change", "change_last"):
        at = e["at"]
        assert at == (nb - 1 if kind == "change_last" else e["key"][1] + e["key"][2])
        assert at >= 1 and not unused[at, s] and not unused[at - 1, s] and seeds[at, s], e
        assert d["carr_phase"][at, s] != d["carr_phase"][at - 1, s], e
    elif "run" in e:
        lo, hi = e["run"]
        assert hi > lo and unused[lo:hi, s].all(), e
        assert lo == 0 or not unused[lo - 1, s], e
        if hi < nb:                                                      # back with the satellite it had: this must seed again
            assert seeds[hi, s], e
            assert lo == 0 or prn[hi, s] == prn[lo - 1, s], e
        B = e["key"][1] if len(e["key"]) > 1 else None
        if kind == "unused_end":
            assert hi == B
        elif kind == "unused_start":
            assert lo == B
        elif kind == "unused_straddle":
            assert lo < B < hi
        elif kind == "unused_long":
            assert hi - lo > 256 and any(lo <= c and c + 256 <= hi for c in range(0, nb, 256)), e
        elif kind == "unused_block0":
            assert lo == 0
        elif kind == "unused_last":
            assert hi == nb
    elif kind == "doppler_zero":
        B = e["key"][1]
        f = d["f_carr"][:, s]
        assert f[B] == 0.0 and np.array_equal(f, (np.arange(nb) - B) * ee.ZERO_SLOPE) and f[B - 1] < 0.0 and (f[B + 1:] > 0.0).all(), e
        assert np.array_equal(d["f_code"][:, s], 1.023e6 + f / 1540.0)
    else:
        assert kind == "exact_tie" and (d["f_carr"][:, s] == FS / 1024.0).all(), e


def check_parts(parts, nb, boundaries, reference):
    """every event that exists is claimed by exactly one part, and every claim is true"""
    expected = ee.edge_events(nb, boundaries, reference)
    want = set(k for k, lo, _, _ in expected if lo is not None and k[0] not in ee.ONE_OF)
    want_kinds = set(k[0] for k, lo, _, _ in expected if lo is not None and k[0] in ee.ONE_OF)
    claimed = []
    for d, rec in parts:
        assert d.shape == (nb, rec["nc"])
        per_slot = {}
        for e in rec["placed"]:
            check_event(d, e)
            claimed.append(e["key"])
            per_slot.setdefault(e["slot"], []).append(e)
        # nothing but the claimed events: a slot without one is plain
        prn, unused, seeds = seeds_and_unused(d)
        for s in range(rec["nc"]):
            if s not in per_slot:
                assert not unused[:, s].any() and seeds[:, s].sum() == 1
    plain = [k for k in claimed if k[0] not in ee.ONE_OF]
    assert len(plain) == len(set(plain)) and set(plain) == want, (want - set(plain), set(plain) - want)
    assert set(k[0] for k in claimed if k[0] in ee.ONE_OF) == want_kinds
    assert not parts[-1][1]["deferred"]
    return want


@pytest.mark.parametrize("nc", [16, 5])
def test_fixed_point_timelines_have_every_event_at_every_boundary(nc):
    """tests 1-3 of the GPU file: thread, wave and round edges of carry_prefix, every piece end of GPSIQ_PIECE_BLOCKS = 1, 3 and
    1024, and the two split points of the continued call"""
    assert ee.piece_ends(ee.NB_FIXED, 1) == [1, 9, 73, 585, 2600] and ee.piece_ends(ee.NB_FIXED, 3) == [3, 27, 219, 1755, 2600]
    assert ee.piece_ends(ee.NB_FIXED, 1024) == [1024, 2600]
    assert set(ee.FIXED_BOUNDARIES) >= {4, 8, 256, 1024, 2048, 1, 9, 73, 585, 3, 27, 219, 1755, 1023}
    want = check_parts(ee.fixed_parts(nc), ee.NB_FIXED, ee.FIXED_BOUNDARIES, False)
    for B in ee.FIXED_BOUNDARIES:
        for key in [("change", B, 0), ("change", B, 1), ("unused_end", B), ("unused_start", B), ("unused_straddle", B)] + [("change", B, -1)] * (B > 1):
            assert key in want, key
    assert {("unused_block0",), ("unused_last",), ("change_last",)} <= want


@pytest.mark.parametrize("nc", [16, 1])
def test_reference_timelines_have_every_event_and_break_the_map(nc):
    """test 4 of the GPU file: the chunk edges of chain_link_scan.  The through-zero slots: the host's certified map of block B is
    refused (ok == 0) at ZERO_SLOPE = 40 Hz per block for B = 256, the first block of a chunk, and B = 511, the last block of one
    (1.5 Hz per block, the slope of the long-block tests, makes nearly every block of 2 048 samples a slow one: the whole slot
    would be refused, and the scan would never see a refused block next to linked ones).  64 blocks away every map is certified."""
    parts = ee.reference_parts(nc)
    want = check_parts(parts, ee.NB_REFERENCE, ee.REFERENCE_BOUNDARIES, True)
    assert {("doppler_zero", 256), ("doppler_zero", 511), ("exact_tie",)} <= want
    for B in ee.REFERENCE_BOUNDARIES:
        for off in (-1, 0, 1):
            assert ("change", B, off) in want
    zeros = 0
    for d, rec in parts:
        for e in rec["placed"]:
            if e["key"][0] == "doppler_zero":
                maps, _ = gpsiq.chain_maps(gpsiq.chain_inputs(d), FS, ee.NS_REFERENCE)
                ok = maps["ok"][:, e["slot"]]
                assert ok[e["zero_at"]] == 0, (e, ok[e["zero_at"] - 3:e["zero_at"] + 4])
                far = (np.abs(np.arange(len(ok)) - e["zero_at"]) > 64) & (d["prn"][:, e["slot"]] > 0)
                assert (ok[far] != 0).all(), np.flatnonzero(far & (ok == 0))
                zeros += 1
    assert zeros == 2


@pytest.mark.parametrize("nb", ee.SHORT_BLOCKS)
@pytest.mark.parametrize("nc", [1, 16])
def test_short_timelines_claim_what_they_hold(nb, nc):
    check_parts(ee.short_parts(nb, nc), nb, ee.SHORT_BOUNDARIES, True)


def chain_agrees(orc, d, ns):
    """float_reference's start and end states == gpsiq.reference_chain's, bit for bit.  (A slot whose last block is unused: the
    serial chain reports satellite 0 and state 0 there; the batch call hands out that block's carr_phase, gpsiq_evaldev.cpp, and
    so does float_reference.)"""
    _, starts, end = ee.float_reference(orc, d, FS, ns, SC08)
    s2, e2, last = gpsiq.reference_chain(gpsiq.chain_inputs(d), FS, ns)
    assert starts.tobytes() == s2.tobytes()
    on = d["prn"][-1] > 0
    assert np.array_equal(last, np.maximum(d["prn"][-1], 0))
    assert end[on].tobytes() == e2[on].tobytes()
    assert end[~on].tobytes() == d["carr_phase"][-1][~on].tobytes() and not e2[~on].any()
    return int(on.sum()), int((~on).sum())


def test_float_reference_is_the_serial_chain(oracle):
    on = off = 0
    for nc in (16, 1):
        for d, _ in ee.reference_parts(nc):
            a, b = chain_agrees(oracle, d, ee.NS_REFERENCE)
            on, off = on + a, off + b
    for nb in ee.SHORT_BLOCKS:
        for d, _ in ee.short_parts(nb, 16):
            chain_agrees(oracle, d, ee.NS_SHORT)
    d, _ = ee.class_timeline(ee.NB_CLASS)
    chain_agrees(oracle, d, ee.NS_CLASS)
    assert on > 0 and off > 0


@pytest.mark.parametrize("ss", [SC08, SC16])
def test_float_reference_is_the_reference_loop(oracle, ref, ss):
    """one short case at the reference's own block length: events on both sides of blocks 2 and 4, four channels"""
    fs = 2600000
    d, rec = ee.edge_timelines(7, 4, (2, 4), 41)[0]
    assert len(rec["placed"]) >= 4
    want, _, carr = ref.run_blocks(d, fs, ss, SINK_IQFILE)
    got, starts, end = ee.float_reference(oracle, d, float(fs), fs // 10, ss)
    assert np.array_equal(got.reshape(-1), want)
    on = d["prn"][-1] > 0
    assert end[on].tobytes() == carr[-1][on].tobytes()


@pytest.mark.parametrize("nc", [16, 5])
def test_fixed_reference_is_the_sequential_oracle(oracle, nc):
    d, _ = ee.fixed_parts(nc)[0]
    q = oracle.quantize_blocks(d, FS, ee.NS_FIXED)
    for ss in (SC08, SC16):
        want = ee.fixed_reference(oracle, d, FS, ee.NS_FIXED, ss)
        for b in (0, d.shape[0] - 1):
            assert np.array_equal(want[b], oracle.block_fixed(q[b], ee.NS_FIXED, ss, seq=True))


def test_class_timeline_puts_each_maximum_in_one_block():
    d, where = ee.class_timeline(ee.NB_CLASS)
    nb = d.shape[0]
    assert nb % 8 != 0 and where["active"] == nb - 1 and len(set(where.values())) == 3
    active = (d["prn"] > 0).sum(axis=1)
    amp = np.where(d["prn"] > 0, (250.0 * np.abs(d["gain"])).astype(np.int64), 0).sum(axis=1)
    step = np.where(d["prn"] > 0, d["f_code"] / FS, 0.0).max(axis=1)
    assert active[where["active"]] == 13 and (np.delete(active, where["active"]) <= 4).all() and active.min() >= 1
    assert amp[where["amp"]] > 32767 and (np.delete(amp, where["amp"]) <= 13 * 250).all()         # (gains of synth_blocks are <= 1)
    # the row kernels' limits (csrc/gpsiq_launch_plan.h): 31/63 chip per sample for seg, 1 for segh
    assert 31.0 / 63.0 < step[where["step"]] <= 1.0 and (np.delete(step, where["step"]) < 31.0 / 63.0).all()
    for head in ee.CLASS_PIECES:
        ends = ee.piece_ends(nb, head)
        assert all(b >= (ends[-2] if len(ends) > 1 else 0) for b in where.values()), "the heavy blocks lie in the last piece"
    assert ee.piece_ends(nb, 16) == [16, 203] and ee.piece_ends(nb, 8) == [8, 72, 203]


def test_patchy_timeline_has_more_patches_than_the_first_copy():
    """the device-evaluated call copies the first 1 024 patches back with its results and the rest in a second copy"""
    d = ee.patchy_timeline(ee.NB_PATCHY, 16)
    patches = gpsiq.reference_blocks(d, FS, ee.NS_PATCHY)[1]
    assert len(patches) > 1024, len(patches)
    assert len(patches) % 64 != 0                                          # the last wave of apply_patches is partly full
    assert len(patches) < 1 << 16                                          # (and the list does not overflow: no fall-back)
