"""The planner of gpsiq_agc / gpsiq_generate_batch_agc (csrc/gpsiq_agc_plan.h through tests/agc_plan.cpp, plain and under
-fsanitize=address,undefined) over the shapes the device tests use and up to the largest span: windows and fill against the contract's
formulas, grids against the geometry, the scratch laid out without overlap; the gain rule of csrc/gpsiq_agc_geometry.h -- the function
the gains kernel evaluates -- against tests/_agc_ref.py; the piece size of the batch call."""
import numpy as np
import pytest

import _agc_plan as ap
import _agc_ref as ar

SANITIZE = pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])


@SANITIZE
def test_plans_hold_their_invariants_everywhere(sanitize):
    lim = ap.ask([("limits",)], sanitize)[0]
    assert lim.threads == 256 and lim.unit == 8 and lim.tile == lim.threads * lim.unit and lim.apply_tile % lim.tile == 0
    assert lim.tile_windows == lim.tile // 64 + 1 and lim.lead_units * lim.unit == 1024 and lim.lead_units <= lim.threads
    sizes = [1, 7, 8, 9, 63, 64, 65, 127, 128, 129, lim.tile - 1, lim.tile, lim.tile + 1, lim.apply_tile - 1, lim.apply_tile, lim.apply_tile + 1,
             700, 26_000_000, 1 << 27, 2 ** 31 - 1]
    reqs = [("plan", n, W, fill, mask) for n in sizes for W in (64, 128, 192, 1024, 65536) for fill in (0, 1, W - 1) for mask in (0, 1)]
    for r, p in zip(reqs, ap.ask(reqs, sanitize)):
        _, n, W, fill, mask = r
        assert p is not None and (p.nwin, p.next) == ar.span(n, W, fill), r
        assert p.measure == -(-n // lim.tile) and p.apply == -(-n // lim.apply_tile) and p.gains == -(-p.nwin // lim.threads), r
        assert p.units == -(-n // lim.unit) and p.scratch - p.mask == (p.units if mask else 0), r
    # nothing to launch: no sample, or a request outside the contract
    assert ap.ask([("plan", 0, 64, 0, 0), ("plan", 0, 1024, 5, 1), ("plan", 10, 32, 0, 0), ("plan", 10, 65537, 0, 0), ("plan", 10, 64, 64, 0)], sanitize) == [None] * 5
    spans = [("span", n, W, fill) for n in (0, 1, 63, 64, 700, 2 ** 40) for W in (64, 192, 65536) for fill in (0, 1, W - 1)]
    for (_, n, W, fill), s in zip(spans, ap.ask(spans, sanitize)):
        assert tuple(s) == ar.span(n, W, fill)


@SANITIZE
def test_the_kernels_gain_rule_is_the_restatements(sanitize):
    rng = np.random.default_rng(12)
    c = ar.cfg(target_q8=210, mult0=999, mult_min=3, mult_max=(1 << 24) - 1)
    pairs = [(0, 0), (0, 1), (0, 1 << 23), (1 << 53, 1 << 23), (2 << 30, 2), (1, 1 << 23), ((1 << 53) - 1, (1 << 23) - 1)]
    for _ in range(3000):
        n = int(rng.integers(1, (1 << 23) + 1))
        pairs.append((int(rng.integers(0, (n << int(rng.integers(0, 31))) + 1)), n))
    reqs = [("gain", S, n, c.target_q8, c.mult0, c.mult_min, c.mult_max) for S, n in pairs]
    for (S, n), g in zip(pairs, ap.ask(reqs, sanitize)):
        assert g == ar.mult(c, S, n), (S, n)


@SANITIZE
def test_piece_sizes(sanitize):
    got = ap.ask([("piece", 0, 4096, 8192, 0), ("piece", 7, 4096, 8192, 0), ("piece", 7, 4096, 8192, 3), ("piece", 7, 4096, 8192, 99),
                  ("piece", 4130, 260000, 520000, 0), ("piece", 100, 2 ** 31 - 1, 2 * (2 ** 31 - 1), 50), ("piece", 5000, 1 << 20, 1 << 21, 4000)], sanitize)
    assert got == [0, 7, 3, 7, 65, 1, 2047]                          # 32 MiB of source; a piece's samples fit an int whatever was asked
