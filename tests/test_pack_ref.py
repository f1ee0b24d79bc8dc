"""The packed stream formats on the CPU: tests/_pack_ref.py (the numpy restatement the GPU tests compare every byte with) against
the contract of include/gpsiq_rows.h ("Packed streams") -- hand-written bytes, round trips over every value -- the library's
gpsiq_packed_block_bytes, the planner of the calls (tests/pack_plan.cpp, also under ASan + UBSan) and the argument checks of
gpsiq_runahead --pack that need no device."""
import os
import subprocess

import numpy as np
import pytest

import _pack_plan as pp
import _pack_ref as pr
import gpsiq
from gpsiq.abi import PK2, PK4, SC08, SC16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_MAX = 2 ** 31 - 1
FORMATS = [(ss, bits) for ss in (SC08, SC16) for bits in (PK4, PK2)]


# ---- the formats ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [PK4, PK2])
@pytest.mark.parametrize("dtype", [np.int8, np.int16])
def test_round_trip_is_the_clamp_for_every_value_in_every_position(bits, dtype):
    """unpack(pack(x)) == clip(x) over all 256 int8 / 65 536 int16 values as I and as Q, in an even and in an odd sample"""
    info = np.iinfo(dtype)
    vals = np.arange(info.min, info.max + 1, dtype=np.int64)
    q = pr.qmax(bits)
    outside = int(np.count_nonzero(np.abs(vals) > q))
    for pos in range(4):                                       # I of sample 0, Q of sample 0, I of sample 1, Q of sample 1
        for other in (0, -q, q):
            x = np.full((len(vals), 6), other, dtype=dtype)    # three samples: an odd count, the last byte of PK2 half used
            x[:, pos] = vals
            p, clipped = pr.pack(x, bits)
            assert p.shape == (len(vals), pr.packed_block_bytes(3, bits)) and p.dtype == np.uint8
            assert clipped == outside
            back = pr.unpack(p, 3, bits, dtype)
            assert back.dtype == dtype and np.array_equal(back, np.clip(x, -q, q))
            if bits == PK2:
                assert not (p[:, -1] >> 4).any()                # odd nsamp: the last byte's high nibble is 0


def test_field_layout_by_hand():
    assert pr.pack(np.array([-7, 3], dtype=np.int8), PK4)[0].tolist() == [0x39]                 # I = -7 -> 9, Q = 3 -> 3 << 4
    assert pr.pack(np.array([1, -1, 0, 1], dtype=np.int8), PK2)[0].tolist() == [0x4D]          # nib0 = 1 | 3 << 2, nib1 = 0 | 1 << 2
    assert pr.pack(np.array([1, -1, 0, 1, -1, 1], dtype=np.int16), PK2)[0].tolist() == [0x4D, 0x07]
    assert pr.unpack([0x39], 1, PK4).tolist() == [-7, 3] and pr.unpack([0x4D, 0x07], 3, PK2).tolist() == [1, -1, 0, 1, -1, 1]
    # saturation is symmetric and counted: -128 -> -7 (never the code of -8), 127 -> 7
    p, n = pr.pack(np.array([-128, 127, -8, 8], dtype=np.int8), PK4)
    assert p.tolist() == [0x79, 0x79] and n == 4 and 0x8 not in (p & 15).tolist() + (p >> 4).tolist()
    p, n = pr.pack(np.array([-2, 2, -1, 1], dtype=np.int8), PK2)
    assert p.tolist() == [0x77] and n == 2


def test_packed_block_bytes_of_the_library_is_the_references():
    ns = list(range(0, 1001)) + [INT_MAX - 2, INT_MAX - 1, INT_MAX, -1, -INT_MAX]
    for bits in (PK4, PK2, 0, 3, 8):
        assert [gpsiq.packed_block_bytes(n, bits) for n in ns] == [pr.packed_block_bytes(n, bits) for n in ns], bits
    assert gpsiq.packed_block_bytes(INT_MAX, PK2) == 2 ** 30 and gpsiq.packed_block_bytes(7, PK2) == 4 and gpsiq.packed_block_bytes(7, PK4) == 7


# ---- the planner ----------------------------------------------------------------------------------------------------------------

SIZES = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4095, 70001, 260000, INT_MAX - 1, INT_MAX]


def plan_requests():
    req = []
    for ss, bits in FORMATS:
        for n in SIZES:
            for nb in (1, 2, 5, 4130, INT_MAX):
                req += [("pack", nb, n, ss, bits), ("unpack", nb, n, bits, ss)]
    return req


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_grids_cover_every_byte_once(sanitize):
    """(the program itself refuses a plan whose units do not tile the block or whose tiles do not tile the units; here: the numbers)"""
    req = plan_requests()
    for r, p in zip(req, pp.ask(req, sanitize)):
        pack = r[0] == "pack"
        nb, n = r[1], r[2]
        ss, bits = (r[3], r[4]) if pack else (r[4], r[3])
        wide, packed = 2 * n * ss, pr.packed_block_bytes(n, bits)
        unit_wide, unit_packed = (p.unit_src, p.unit_dst) if pack else (p.unit_dst, p.unit_src)
        assert unit_wide * bits == unit_packed * 8 * ss                   # a unit's two sides are the same elements
        assert p.units == -(-wide // unit_wide) and (p.units - 1) * unit_packed < packed <= p.units * unit_packed
        assert p.tiles == -(-p.units // (p.threads * 4)) and p.total == p.tiles * nb and p.grid == min(p.total, 1 << 20)
        assert unit_wide % 16 == 0 and unit_packed % 4 == 0 and p.threads == 256
    # nothing to do, or no such format: no launch
    none = [("pack", 0, 100, 1, 4), ("pack", 3, 0, 1, 4), ("pack", -1, 100, 2, 2), ("unpack", 3, -5, 4, 1), ("pack", 3, 100, 4, 4), ("pack", 3, 100, 1, 3),
            ("unpack", 3, 100, 8, 1)]
    assert pp.ask(none, sanitize) == [None] * len(none)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_pieces_tile_the_call_and_the_override_is_honoured(sanitize):
    cases = [(nb, blk, ov) for nb in (1, 2, 7, 40, 4130, INT_MAX) for blk in (0, 2, 5200, 520000, 5000000, 2 ** 32 - 4, 2 ** 33)
             for ov in (0, -3, 1, 7, 64, 10 ** 9)]
    got = pp.ask([("piece",) + c for c in cases] + [("bytes", n, b) for n in (INT_MAX, INT_MAX - 1, 0, -1) for b in (4, 2, 3)], sanitize)
    for (nb, blk, ov), piece in zip(cases, got):
        assert 1 <= piece <= nb
        if ov > 0:
            assert piece == min(ov, nb)                                    # the override, as far as the call goes
        elif blk:
            assert piece == min(nb, max(1, -(-(32 << 20) // blk)))       # ~32 MiB of source, at least one block
        # the pieces [k * piece, min((k + 1) * piece, nb)) tile [0, nb): as many as the division says, the last one ragged
        k = -(-nb // piece)
        assert (k - 1) * piece < nb <= k * piece
    assert got[len(cases):] == [pr.packed_block_bytes(n, b) for n in (INT_MAX, INT_MAX - 1, 0, -1) for b in (4, 2, 3)]
    assert pp.ask([("piece", 40, 5200, 7)], sanitize) == [7] and pp.ask([("piece", 4130, 520000, 0)], sanitize) == [65]


# ---- gpsiq_runahead --pack: the checks that need no device ---------------------------------------------------------------------

def runahead(*flags, sample_size="1"):
    exe = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "host", "gpsiq_runahead")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.dirname(exe)], check=True)
    args = [exe, "no-such-rinex", "2", "2190", "270000", "0,0,0", "1", "8", "2600000", sample_size, "out.bin"]
    return subprocess.run(args + list(flags), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flags", [("--pack", "4"), ("--level", "2.3", "--qmax", "8", "--pack", "4"), ("--level", "0.6", "--qmax", "7", "--pack", "2"),
                                   ("--level", "0.6", "--qmax", "2", "--pack", "2"), ("--level", "2.3", "--pack", "3"), ("--pack", "2", "--cn0", "45")],
                         ids=lambda f: " ".join(f))
def test_runahead_pack_refuses_what_the_format_cannot_hold(flags):
    r = runahead(*flags)
    assert r.returncode == 2 and "usage:" in r.stderr and "--pack 4|2" in r.stderr, (r.returncode, r.stderr)


def test_runahead_pack_needs_sample_size_1_and_accepts_the_rest():
    r = runahead("--level", "2.3", "--pack", "4", sample_size="2")
    assert r.returncode == 2 and "usage:" in r.stderr
    # well-formed: past the argument checks, stopped by the RINEX file that is not there
    for flags in (("--level", "2.3", "--pack", "4"), ("--level", "2.3", "--qmax", "5", "--pack", "4"), ("--level", "0.6", "--pack", "2", "--cn0", "45")):
        r = runahead(*flags)
        assert r.returncode == 1 and "cannot read" in r.stderr, (flags, r.returncode, r.stderr)
