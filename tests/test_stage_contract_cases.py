"""The cases of tests/_contract_cases.py held to their names on the CPU, and the new entries of the restatements held to the old ones:
acquire_windows (dwell windows with their absolute first samples) against the dense acquire and, at hops no dense array can hold,
against sums written out sample by sample; follow_rebased against follow on the whole stream.  What the GPU tests of stream order, wide
offsets, peak ties and 32 followed satellites rely on -- that an all-0x7f input gives another answer, that the layouts cross 2^31 and
2^32 where they say, that the ties are there and where, which status each satellite stops with -- is asserted here."""
import numpy as np
import pytest

import _acquire_plan as ap
import _acquire_ref as ar
import _contract_cases as cc
import _follow_plan as fp
import _follow_ref as fr
import _oracle
from gpsiq.abi import FOLLOW_STATE_DTYPE, SC08, SC16


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the new entries of the restatements ------------------------------------------------------------------------------------------------

def dense_search(rng, hop, ss=SC16):
    nshift, ncoh, nn = 300, 128, 2
    info = np.iinfo(np.int16 if ss == SC16 else np.int8)
    stream = rng.integers(info.min, info.max + 1, size=2 * ap.span_of(nshift, ncoh, nn, hop)).astype(info.dtype)
    width = nshift - 1 + ncoh
    return stream, [stream[2 * k * hop:2 * (k * hop + width)] for k in range(nn)], [k * hop for k in range(nn)], (nshift, ncoh)


def test_the_windowed_search_equals_the_dense_one(orc):
    """hop 5000: two dwell windows of 427 samples out of 5427, both formats, bins whose carrier depends on the absolute sample"""
    for ss in (SC16, SC08):
        stream, wins, first, (nshift, ncoh) = dense_search(np.random.default_rng(40 + ss), 5000, ss)
        dense = ar.acquire(orc, stream, (9, 27), *cc.WIDE_STEPS, 3, nshift, ncoh, 2, 5000)
        assert same_bytes(ar.acquire_windows(orc, wins, first, (9, 27), *cc.WIDE_STEPS, 3, nshift, ncoh), dense)
        # a window taken at another absolute sample is another search: the carrier index is at absolute m
        moved = ar.acquire_windows(orc, wins, [0, 4999], (9, 27), *cc.WIDE_STEPS, 3, nshift, ncoh)
        assert moved[2][:, :, 0].tobytes() == dense[2][:, :, 0].tobytes() and moved[2][:, :, 1].tobytes() != dense[2][:, :, 1].tobytes()


def test_samples_between_the_dwell_windows_are_no_input(orc):
    stream, wins, first, (nshift, ncoh) = dense_search(np.random.default_rng(43), 5000)
    before = ar.acquire(orc, stream, (9, 27), *cc.WIDE_STEPS, 3, nshift, ncoh, 2, 5000)
    other = stream.copy()
    other[2 * (nshift - 1 + ncoh):2 * 5000] = cc.guard_elements(2 * (5000 - (nshift - 1 + ncoh)), SC16)
    assert other.tobytes() != stream.tobytes() and same_bytes(ar.acquire(orc, other, (9, 27), *cc.WIDE_STEPS, 3, nshift, ncoh, 2, 5000), before)


def test_the_sum_written_out_from_a_window_equals_the_one_from_the_stream(orc):
    stream, wins, first, (nshift, ncoh) = dense_search(np.random.default_rng(44), 5000)
    for d, s, k in [(0, 0, 0), (2, 299, 1), (1, 17, 1)]:
        step = cc.WIDE_STEPS[1] + d * cc.WIDE_STEPS[2]
        assert ar.acquire_direct_window(orc, wins[k], first[k], 27, cc.WIDE_STEPS[0], step, s, ncoh) == ar.acquire_direct(orc, stream, 27, cc.WIDE_STEPS[0], step, s, k, 5000, ncoh)


@pytest.mark.parametrize("name", [w.name for w in cc.WIDE_SEARCHES])
def test_the_wide_searches_against_sums_written_out(orc, name):
    """a dozen cells of each wide search, both dwells, every bin, first and last shift: Python integers at the absolute sample"""
    w, wins, first, (peaks, power, corr) = cc.wide_search_reference(name)
    cells = [(p, d, k, s) for p in (0, 1) for d in (0, 2) for k in (0, 1) for s in ((0, 299) if (p + d // 2 + k) & 1 else (150,))]
    assert len(cells) == 12
    for p, d, k, s in cells:
        want = ar.acquire_direct_window(orc, wins[k], first[k], w.prns[p], cc.WIDE_STEPS[0], cc.WIDE_STEPS[1] + d * cc.WIDE_STEPS[2], s, w.ncoh)
        assert want == (int(corr["i"][p, d, k, s]), int(corr["q"][p, d, k, s])), (p, d, k, s)
    xi, xq = corr["i"].astype(np.float64), corr["q"].astype(np.float64)
    assert np.array_equal(power, (0.0 + (xi[:, :, 0] ** 2 + xq[:, :, 0] ** 2)) + (xi[:, :, 1] ** 2 + xq[:, :, 1] ** 2))
    assert np.array_equal(peaks["shift"], power.argmax(axis=2)) and power.min() > 0.0


def test_the_rebased_run_equals_the_run_on_the_whole_stream(orc):
    """B = 5000: follow on stream[2 B:] with B added back to every sample -- records, counts and states of the run on the whole stream"""
    B = 5000
    case = cc.by_name(fp.CASES, "mixed-int16")
    stream = fr.case_stream(case, 0)[:2 * (B + 9000)]
    cfg = fr.make_cfg(**case.cfg)
    states = np.array([fr.make_state(**s) for s in case.states], dtype=FOLLOW_STATE_DTYPE)
    states["sample"] += np.uint64(B)
    whole = fr.follow(orc, stream, cfg, states, 64)
    assert min(whole[1]) > 10 and all(s == fr.SPAN_END for s in whole[2]["status"])
    assert same_bytes(fr.follow_rebased(orc, stream[2 * B:], B, cfg, states, 64), whole)


# ---- A. stream order --------------------------------------------------------------------------------------------------------------------

def test_an_input_of_0x7f_gives_another_answer_in_every_stream_order_case():
    """what the buffer holds until the producer has run, and what the context's buffers hold from the ordinary call before: every output
    the GPU test compares differs from the expected one"""
    for name in cc.STREAM_DESPREAD:
        c, q, stream, ref = cc.despread_reference(name)
        wrong = cc.despread_of_guard(name)
        assert c.kernel == ("generic" if "generic" in name else "rows") and c.nblocks >= 2
        assert wrong[0].tobytes() != ref[0].tobytes() and wrong[2].tobytes() != ref[2].tobytes() and np.array_equal(wrong[1], ref[1])
        assert all(np.any(wrong[0][b] != ref[0][b]) for b in range(c.nblocks))
    for name in cc.STREAM_ACQUIRE:
        c = cc.by_name(ap.CASES, name)
        wrong, ref = cc.acquire_of_guard(name), cc.acquire_reference(name)[2]
        assert all(w.tobytes() != r.tobytes() for w, r in zip(wrong, ref))
        assert np.all(wrong[0]["power"] != ref[0]["power"])
    assert ap.full_tile(*[(c.ndopp, c.nshift) for c in ap.CASES if c.name == cc.STREAM_ACQUIRE[0]][0])
    assert not ap.full_tile(*[(c.ndopp, c.nshift) for c in ap.CASES if c.name == cc.STREAM_ACQUIRE[1]][0])
    for name in cc.STREAM_FOLLOW:
        c, stream, cfg, states, ref = cc.follow_reference(name)
        wrong = cc.follow_of_guard(name)
        assert wrong[0].tobytes() != ref[0].tobytes() and wrong[2].tobytes() != ref[2].tobytes()
        # relaunches: more than two launches of STREAM_FOLLOW_KNOB epochs
        assert int(max(ref[1])) // cc.STREAM_FOLLOW_KNOB + 1 > 2
        for p in range(len(states)):
            assert any(np.any(wrong[0][p][f] != ref[0][p][f]) for f in fr.SUMS)
    for ss, bits in cc.PACK_FORMATS:
        x, packed, count, back = cc.pack_reference(ss, bits)
        assert x.shape == (5, 2 * 70001)
        wrong = cc.pack_of_guard(ss, bits)
        assert wrong[1] != count and all(np.any(wrong[0][b] != packed[b]) for b in range(5)) and all(np.any(wrong[2][b] != back[b]) for b in range(5))


# ---- B. wide offsets ----------------------------------------------------------------------------------------------------------------------

def test_the_wide_layouts_cross_2_31_and_2_32_where_stated(orc):
    W = cc.WIDE_STRIDE
    assert (2 * W, 4 * W) == (2 ** 31 + 8, 2 ** 32 + 16) and W % 4 == 0 and cc.WIDE_BLOCKS == 5
    # a truncated offset of block 2 or 4 lands inside block 0 for every block length the wide tests use (at least 513 bytes)
    assert (2 * W) % 2 ** 31 == 8 and (4 * W) % 2 ** 32 == 16 and (4 * W) % 2 ** 31 == 16
    assert cc.wide_bytes(4 * 4999) == 4 * W + 4 * 4999 + 64
    w16, w8 = cc.WIDE_SEARCHES
    assert (w16.ss, w8.ss) == (SC16, SC08)
    for w in cc.WIDE_SEARCHES:
        assert ap.span_of(w.nshift, w.ncoh, w.nnoncoh, w.hop) == w.nsamp <= 2 ** 31 - 1 and (w.nshift, w.ncoh, w.nnoncoh, w.ndopp, len(w.prns)) == (300, 128, 2, 3, 2)
        # the digit planes exceed the scratch cap: generic whatever is asked
        for force in (None, "mfma", "generic"):
            plan = ap.query(w.nsamp, w.ss, len(w.prns), w.ndopp, w.nshift, w.ncoh, w.nnoncoh, w.hop, force)
            assert plan.kernel == "generic" and plan.span == w.nsamp
    assert w16.hop * 4 > 4.79e9 and w16.hop * 4 > 2 ** 32          # the second dwell's first byte
    assert w8.nsamp == 2 ** 31 - 1 and 2 * w8.hop > 2 ** 31 and 2 * w8.hop < 2 ** 32      # element indices past 2^31
    # at 2.6 Msps the carrier of the outer bins turns thousands of times over the span: the index at absolute m is not the local one
    assert not np.array_equal(ar.carrier_index_from(cc.WIDE_STEPS[1], w16.hop, 427), ar.carrier_index(cc.WIDE_STEPS[1], 427))


def test_the_wide_follow_ends_on_a_record_s_last_sample():
    nsamp, base, tail, cfg, states, ref = cc.wide_follow_reference()
    assert nsamp == cc.WIDE_SEARCHES[0].hop and base + len(tail) // 2 == nsamp and 4 * base > 2 ** 32
    assert [int(s) for s in ref[2]["status"]] == [fr.SPAN_END] * 2 and list(ref[1]) == [4, 4]
    last = ref[0][0, 3]
    assert int(last["sample"]) + int(last["nsamp"]) == nsamp == int(ref[2][0]["sample"]) and int(ref[2][1]["sample"]) < nsamp
    assert all(2600 < nsamp - int(s) < 3100 for s in states["sample"]) and all(int(c) == 3 << 55 for c in states["code_step0"])
    assert all(660 < int(n) < 700 for n in ref[0]["nsamp"][0, :4])


# ---- C. peak ties -------------------------------------------------------------------------------------------------------------------------

def test_the_tie_cases_hold_the_ties_their_names_promise():
    assert [(t.ss, t.period, t.nshift, t.ncoh, t.nnoncoh, t.hop) for t in cc.TIES] == [(SC16, 100, 700, 128, 2, 333), (SC08, 64, 300, 64, 1, 64), (SC16, 16, 257, 64, 3, 50)]
    assert [t.name for t in cc.TIES] == ["p100-int16", "p64-int8", "p16-int16"] and cc.TIE_STEPS[1] == 0 and cc.TIE_STEPS[2] != 0
    counts = []
    for t in cc.TIES:
        _, stream, (peaks, power, corr) = cc.tie_reference(t.name)
        x = stream.reshape(-1, 2)
        assert len(t.prns) == 2 and t.ndopp == 2 and np.array_equal(x[t.period:], x[:-t.period])
        for p in range(2):
            s = int(peaks["shift"][p, 0])
            at = np.flatnonzero(power[p, 0] == peaks["power"][p, 0])
            assert 1 <= s < t.period
            assert list(at) == list(range(s, t.nshift, t.period)) and len(at) == -(-(t.nshift - s) // t.period) >= 4
            # the X themselves repeat, dwell by dwell
            assert all(corr[p, 0, :, a].tobytes() == corr[p, 0, :, s].tobytes() for a in at)
            assert np.count_nonzero(power[p, 1] == peaks["power"][p, 1]) == 1       # bin 1: no tie
            counts.append(len(at))
    assert counts == [7, 7, 5, 5, 16, 16]


# ---- D. thirty-two satellites -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [SC08, SC16])
def test_the_thirty_two_satellites_stop_as_pinned(ss):
    stream, cfg, states, ref = cc.follow32_reference(ss)
    assert sorted(int(p) for p in states["prn"]) == list(range(1, 33)) and ref[0].shape == (32, 12)
    assert len(set(int(s) for s in states["sample"])) == 32 and len(set(int(c) for c in states["chip"])) == 32 and len(set(int(f) for f in states["code_frac"])) == 32
    assert (states["carr_step"] > 0).sum() == 16 and (states["carr_step"] < 0).sum() == 16
    status = tuple(int(s) for s in ref[2]["status"])
    assert status == cc.FOLLOW32_EXPECT[ss] and set(status) == {fr.SPAN_END, fr.FULL, fr.RANGE}
    # launches of FOLLOW32_KNOB epochs: satellites stop in the first, the second and the third
    assert {int(n) // cc.FOLLOW32_KNOB for n in ref[1]} == {0, 1, 2} and int(max(ref[1])) == 12
    plan = fp.query(len(stream) // 2, ss, 32, 12, cc.FOLLOW32_KNOB, 12)
    assert (plan.grid, plan.per_launch, plan.launches) == (32, 5, 3)
    # the used context's large call: every record slot of the first satellite filled
    big = cc.follow32_reference(SC16, 48000, 64)[3]
    assert int(max(big[1])) == 64 and int(min(big[1])) >= 1 and fr.FULL in big[2]["status"]
