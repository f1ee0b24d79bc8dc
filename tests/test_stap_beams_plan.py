"""The planner of gpsiq_stap_beams over its whole range, the digit planes of the matrix kernel multiplied out against the weights, and
one chunk of that kernel modelled on the CPU against the direct sums (tests/stap_beams_plan.cpp), plain and under ASan and UBSan."""
import itertools

import pytest

import _stap_beams_plan as bp

SHAPES = [(e, t) for e in range(1, 9) for t in range(1, 9) if e * t <= 32]
ENTRIES = (-32768, 0, 32639, 32640, 32767)


def all_plans(sanitize=False):
    reqs = [("plan", e, t, b, nsamp, ins, out, entry, force) for (e, t) in SHAPES for b in range(1, 9) for ins in (1, 2) for out in (1, 2) for entry in ENTRIES
            for force in (bp.AUTO, bp.FORCE_GENERIC, bp.FORCE_MFMA) for nsamp in (0, 1, 513, 5_000_000)]
    return reqs, bp.ask(reqs, sanitize)


def test_a_kernel_is_named_for_every_legal_shape_and_forced_kernels_are_refused_only_where_they_cannot_serve():
    lim = bp.limits()
    assert lim.max_entry == 127 * 256 + 127 and lim.max_beams == 8 and (lim.chunk8, lim.chunk16) == (4 * lim.tile8, 4 * lim.tile16) == (512, 256)
    reqs, plans = all_plans()
    seen = set()
    for (_, e, t, b, nsamp, ins, out, entry, force), p in zip(reqs, plans):
        if nsamp == 0:
            assert p is None
            continue
        tp = bp.padded_taps(e, t)
        can = tp > 0 and entry <= lim.max_entry
        assert p.can == can and p.kernel in bp.KERNELS and p.threads == lim.threads
        if force == bp.FORCE_GENERIC:
            assert p.kernel == bp.GENERIC
        elif force == bp.FORCE_MFMA:
            assert p.kernel == (bp.MFMA if can else bp.GENERIC)        # refused only where it cannot serve
        else:
            assert p.kernel == (bp.MFMA if can and bp.default_is_mfma(ins, e * tp, b) else bp.GENERIC)
        if p.kernel == bp.MFMA:
            assert p.padded == tp and t <= tp < 2 * t and e * tp <= 32 and p.run == (lim.chunk8 if out == 1 else lim.chunk16)
            assert p.grid == min(p.runs, lim.max_grid)
        else:
            assert p.padded == 0 and p.grid == min(p.runs, lim.gen_grid)
        assert (p.runs - 1) * p.run < nsamp <= p.runs * p.run
        seen.add((p.kernel, p.padded))
    # every padding decision was met on both sides: shapes that pad (3 -> 4, 5 -> 8), shapes that fit as they are, shapes that cannot pad
    assert seen == {(bp.GENERIC, 0), (bp.MFMA, 1), (bp.MFMA, 2), (bp.MFMA, 4), (bp.MFMA, 8)}
    assert bp.padded_taps(4, 5) == 8 and bp.padded_taps(5, 5) == 0 and bp.padded_taps(8, 4) == 4 and bp.padded_taps(8, 5) == 0 and bp.padded_taps(3, 3) == 4


def test_the_default_is_the_measured_one():
    """the thresholds as csrc/gpsiq_stap_beams_plan.h cites them from profiles/stap_beams_rates.txt; fewer than four beams never"""
    never = bp.limits().never
    assert never > 32
    got = bp.ask([("minrows", ins, b) for ins in (1, 2) for b in range(1, 9)])
    assert got == [never] * 3 + [8] * 4 + [2] + [never] * 3 + [16] * 4 + [8]
    for ins in (1, 2):
        for b in range(1, 9):
            for rows in range(1, 33):
                assert bp.default_is_mfma(ins, rows, b) == (rows >= got[8 * (ins - 1) + b - 1])


def test_every_weight_value_splits_into_planes_that_multiply_out_or_goes_to_the_generic_kernel():
    s = bp.ask([("split", -32768, 32767)])[0]
    assert (s.planes, s.generic) == (32768 + 32640, 32767 - 32639)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_the_planes_multiply_out_against_the_weights(sanitize):
    reqs = [("planes", e, t, b, 7 * e + t + b, kind) for (e, t) in SHAPES if bp.padded_taps(e, t) for b in (1, 2, 3, 7, 8) for kind in (0, 1)]
    assert all(bp.ask(reqs, sanitize))


def tiles():
    reqs = []
    shapes = [(1, 1), (1, 8), (2, 4), (4, 2), (8, 1), (3, 3), (4, 5), (8, 4), (4, 8)]       # (5, 5) does not pad: the generic kernel's
    for k, ((e, t), b, (in_size, out_size)) in enumerate(itertools.product(shapes, (1, 3, 8), ((1, 1), (1, 2), (2, 1), (2, 2)))):
        chunk = 512 if out_size == 1 else 256
        for kind in (0, 1, 2):
            reqs.append(("tile", e, t, b, in_size, out_size, (chunk, chunk - 1, 17, t)[(k + kind) % 4], 1000 + k, kind, (k + kind) % 3))
    return reqs


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_the_modelled_chunk_equals_the_direct_sums_on_random_and_extreme_data(sanitize):
    reqs = tiles()
    got = bp.ask(reqs, sanitize)
    assert all(t.peak <= 2 ** 20 for t in got)
    # the extremes reach the sums the recombination has to carry modulo 2^32: beyond 2^30 for int16 input, where 65536 P11 alone wraps
    assert max(t.acc for r, t in zip(reqs, got) if r[4] == 2 and r[8] == 1) > 2 ** 30
    assert max(t.acc for r, t in zip(reqs, got) if r[4] == 1 and r[8] == 1) > 2 ** 22


def test_the_planner_runs_clean_under_the_sanitizers():
    reqs, plans = all_plans(sanitize=True)
    assert plans == bp.ask(reqs)
    assert bp.ask([("split", -32768, 32767), ("limits",)], sanitize=True) == bp.ask([("split", -32768, 32767), ("limits",)])
