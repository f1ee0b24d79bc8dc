"""The carrier chain's certified maps (csrc/gpsiq_lane.h) audited over their WHOLE range, on the host twin (gpsiq.chain_maps: the
lane code the device shares), and tests/_chain_audit.py held to itself.  Every other chain test pushes the one true start state
through a map -- an offset of a handful of units in a range of 1e12; here a map's claim (start xs + d U, lo <= d <= hi, parity
allowed by ok -> end e + (d + cum[p]) U) is tried at lo, at hi, a grid step inside them, per parity and in between, against the
reference's accumulator (gps.c:2821-2826, restated in numpy: _chain_audit.walk) started from that very state.  No GPU.

Measured on the host maps (max_stretches 1, 5 and 32 each; maps audited / probes kept / skipped / offsets the map does not claim):
    2.6 Msps, the edge timelines of tests/test_gpu_chain_edges.py     267 079 / 2 130 502 / 358 / 3 848
    2^21 sps, the exact-tie timelines                                   3 680 /    28 480 /   0 /   640
    timeline() of test_chain_parallel.py, 2.6 Msps                        666 /     5 328 /   0 /     0
    ... 10 Msps                                                           678 /     5 424 /   0 /     0
    ... 25 Msps                                                           654 /     5 232 /   0 /     0
    ... 2^21 sps                                                          678 /     5 424 /   0 /     0
No probe ended anywhere but where its map says.  ok = 2 never comes out of join_stretches (a descending carrier's top tie closes
the odd branch in stretch 0 already, where the even branch's offset is 0: a map holds for both parities, for the even one, or not
at all), so the odd-only leg of link_block is tried on maps re-based by one grid step (rebased(): the same claim, told from the
neighbouring representative)."""
import numpy as np
import pytest

import gpsiq
import _chain_audit as A
from test_chain_parallel import timeline

STRETCHES = (1, 5, 32)
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def edge_timelines():
    """every part-C timeline: [(name, cin, record, fs, nsamp)]"""
    def make():
        out = [(f"scan{nb}", *A.scan_edge_timeline(nb), A.FS, 600) for nb in A.SCAN_BLOCKS]
        out += [(f"lanes{kseg}x{nb}", *A.lane_edge_timeline(kseg, nb), A.FS, A.NS_LANES) for kseg in A.LANE_SEGS for nb in A.lane_blocks(kseg)]
        out += [(f"lanes32x25@{ns}", *A.lane_edge_timeline(32, 25, nsamp=ns), A.FS, ns) for ns in (1, 7)]
        out += [(f"tie@{ns}", *A.tie_timeline(40, ns), A.FS_TIE, ns) for ns in (A.NS_LANES, 4096)]
        return out
    return _once("edges", make)


# ---- 1. the two references ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsamp", [1, 2, 7, 600, 4096])
def test_serial_end_equals_walk(nsamp):
    rng = np.random.default_rng(nsamp)
    n = 3000
    c = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-7, np.log10(0.5), n)
    bits = c.view(np.uint64).copy()
    z = rng.integers(4, 50, n).astype(np.uint64)
    tie = np.arange(n) % 4 == 0                                      # exact-tie addends: trailing zeros, the lowest bit set
    bits[tie] = (bits[tie] & ~((np.uint64(1) << z[tie]) - np.uint64(1))) | (np.uint64(1) << z[tie])
    c = bits.view(np.float64)
    c[:8] = [0.5 - 2.0 ** -54, -(0.5 - 2.0 ** -54), 0.25, -0.25, 2.0 ** -10, -2.0 ** -10, 0.49999, -0.49999]     # |c| just under 0.5
    x = rng.random(n)
    k = rng.integers(1, 40, n)
    x[1::5] = np.ldexp(1.0 + rng.integers(-2, 3, len(x[1::5])) * 2.0 ** -52, -k[1::5])       # binade edges, a few ulps either side
    x[2::5] = np.abs(c[2::5]) * rng.random(len(x[2::5]))                                     # just after a wrap, climbing
    x[3::5] = 1.0 - np.abs(c[3::5]) * rng.random(len(x[3::5]))                               # ... and descending
    x[:4] = [0.0, 1.0 - 2.0 ** -53, 0.5, 2.0 ** -53]
    x = np.where((x >= 0.0) & (x < 1.0), x, 0.0)
    fs = 2.6e6
    f = c * fs
    keep = np.abs(f * (1.0 / fs)) < 0.5
    x, f = x[keep], f[keep]
    assert keep.sum() > 0.99 * n and (f > 0).sum() > 1000 and (f < 0).sum() > 1000 and np.abs(f * (1.0 / fs)).max() > 0.4999
    want = A.walk(x, f * (1.0 / fs), nsamp)
    got = A.serial_end(x, 1 + np.arange(len(x)) % 32, f, fs, nsamp)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:5]


def test_walk_is_the_plain_loop():
    """walk() against the reference's three lines in a scalar loop"""
    rng = np.random.default_rng(3)
    x0, c = rng.random(40), rng.uniform(-0.49, 0.49, 40)
    want = []
    for x, cc in zip(x0.tolist(), c.tolist()):
        for _ in range(300):
            x += cc
            if x >= 1.0:
                x -= 1.0
            elif x < 0.0:
                x += 1.0
        want.append(x)
    assert A.walk(x0, c, 300).tobytes() == np.array(want).tobytes()


# ---- 2. link_block restated == gpsiq.chain_link ----------------------------------------------------------------------------------------
def test_admits_and_apply_agree_with_chain_link():
    total = 0
    for name, cin, _, fs, nsamp in edge_timelines():
        for ms in (1, 32):
            maps, _ = gpsiq.chain_maps(cin, fs, nsamp, max_stretches=ms)
            before = gpsiq.chain_stats()
            start, end, last = gpsiq.chain_link(cin, maps, fs, nsamp)
            linked = gpsiq.chain_stats()[0] - before[0]
            adm = A.true_admission(maps, cin, start)
            assert adm.sum() == linked, (name, ms, int(adm.sum()), linked)
            nxt = np.vstack([start[1:], end[None, :]])
            cont = np.vstack([(cin["prn"][1:] == cin["prn"][:-1]) & (cin["prn"][1:] > 0), (cin["prn"][-1:] > 0)])      # the next block continues this one
            m = adm & cont
            assert A.apply(maps[m], start[m]).tobytes() == nxt[m].tobytes(), (name, ms)
            total += int(m.sum())
    assert total > 100000


def test_the_quick_way_of_link_is_the_integers_way():
    """link()'s int64 path (states that are whole numbers of 2^-62) == its Python-integer path (whole numbers of 2^-1074), on probes
    of every kind: kept, off the class, outside the range, closed parity, an end that is no double"""
    name, cin, _, fs, nsamp = edge_timelines()[8]
    maps, _ = gpsiq.chain_maps(cin, fs, nsamp, max_stretches=5)
    rec = maps[maps["ok"] != 0][:1500]
    P = A.probes(rec, np.random.default_rng(1), 2)
    R = np.broadcast_to(rec[:, None], P.d.shape)
    x = np.concatenate([P.x.reshape(-1), P.x.reshape(-1) + 2.0 ** -60, P.x.reshape(-1) + 3 * A.U])
    R = np.concatenate([R.reshape(-1)] * 3)
    x = np.where((x >= 0) & (x < 1), x, 0.5)
    a, b = A.link(R, x), A.link(R, x, quick=False)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert set(np.unique(a[0]).tolist()) >= {0, 2, 3}


def rebased(rec):
    """the maps that hold for even offsets only, told from the representative one grid step up: the same claim, for odd offsets only"""
    r = rec[rec["ok"] == 1].copy()
    g = (r["info"] & 0xff).astype(np.int64)
    r["xs"] = r["xs"] + g * A.U
    r["lo"], r["hi"] = r["lo"] - g, r["hi"] - g
    r["cum"] = np.stack([r["cum"][:, 1] + g, r["cum"][:, 0] + g], axis=1)
    r["ok"] = 2
    return r


def test_maps_for_odd_offsets_only():
    cin, _ = A.tie_timeline(40, 4096)
    maps, _ = gpsiq.chain_maps(cin, A.FS_TIE, 4096, max_stretches=1)
    sel = maps["ok"] == 1
    assert sel.sum() >= 40
    r2 = np.zeros(maps.shape, dtype=maps.dtype)
    r2[sel] = rebased(maps[sel])
    assert np.all(r2["ok"][sel] == 2) and np.all((r2["xs"][sel] >= 0) & (r2["xs"][sel] < 1))
    res = A.audit(cin, r2, A.FS_TIE, 4096, np.random.default_rng(2), 4)
    assert res.ok2 == sel.sum() and res.kept >= 6 * res.ok2 and res.odd_at_lo == res.ok2 and res.odd_at_hi == res.ok2, res
    res.assert_caps()
    # ... and gpsiq.chain_link takes them: the chain is the serial chain's, with as many blocks linked
    want = gpsiq.reference_chain(cin, A.FS_TIE, 4096)
    both = maps.copy()
    both[sel] = r2[sel]
    before = gpsiq.chain_stats()
    got = gpsiq.chain_link(cin, both, A.FS_TIE, 4096)
    linked = gpsiq.chain_stats()[0] - before[0]
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes()
    assert linked == A.true_admission(both, cin, want[0]).sum() == A.true_admission(maps, cin, want[0]).sum()


# ---- 3. / 4. the audit of the host twin's maps, and what it reached ---------------------------------------------------------------------
def host_audits():
    def make():
        out = {}
        cases = [(n, c, fs, ns) for n, c, _, fs, ns in edge_timelines()]
        cases += [(f"timeline@{fs:g}", timeline(int(fs) % 997, 40, 6), fs, int(fs / 10)) for fs in (2.6e6, 10e6, 25e6, 2097152.0)]
        for name, cin, fs, nsamp in cases:
            for ms in STRETCHES:
                maps, _ = gpsiq.chain_maps(cin, fs, nsamp, max_stretches=ms)
                out[name, ms] = A.audit(cin, maps, fs, nsamp, np.random.default_rng(len(out)), 2, ms)
        return out
    return _once("audits", make)


def test_the_audit_of_the_host_maps():
    """No probe of any map ends anywhere but where the map says (audit() raises on the first that does), and per timeline and
    max_stretches the caps hold: skipped probes (outside [0, 1) or refused by link_block's exactness checks) at most 10 % of those
    generated, and every map keeps its lo-side and its hi-side probe of one parity."""
    res = host_audits()
    for key, r in res.items():
        r.assert_caps()
    for what, pick in (("2.6 Msps edge timelines", lambda n: n.startswith(("scan", "lanes"))), ("2^21 sps tie timelines", lambda n: n.startswith("tie")),
                       ("timeline() 2.6 Msps", lambda n: n == "timeline@2.6e+06"), ("timeline() 10 Msps", lambda n: n == "timeline@1e+07"),
                       ("timeline() 25 Msps", lambda n: n == "timeline@2.5e+07"), ("timeline() 2^21 sps", lambda n: n == "timeline@2.09715e+06")):
        tot = sum((r for (n, _), r in res.items() if pick(n)), A.Audit())
        print(f"{what}: maps {tot.maps}, probes kept {tot.kept}, skipped {tot.skipped}, not claimed {tot.closed}")
        assert tot.maps > 0 and tot.kept >= 6 * tot.maps, (what, tot)


def test_what_the_audited_host_maps_include():
    """ok = 1 and 3 (2: see the module's docstring and test_maps_for_odd_offsets_only), cum[0] != cum[1], both grids, both signs, maps of
    1 stretch and of 32, odd-parity probes at lo and at hi -- and the long blocks of serial_end as well as the short ones of walk"""
    res = host_audits()
    tot = sum(res.values(), A.Audit())
    assert tot.ok1 > 100 and tot.ok3 > 1000 and tot.ok2 == 0, tot
    assert tot.cum_differ > 100 and tot.grid1 > 1000 and tot.grid2 > 1000 and tot.c_pos > 1000 and tot.c_neg > 1000, tot
    assert {1, 32} <= tot.seg and tot.odd_at_lo > 1000 and tot.odd_at_hi > 1000, tot
    ties = sum((r for (n, _), r in res.items() if n.startswith("tie")), A.Audit())
    assert ties.ok1 > 0 and ties.cum_differ > 100 and ties.odd_at_lo > 100 and ties.odd_at_hi > 100, ties
    for ms in STRETCHES:                                               # the timelines of test_chain_parallel.py: mostly maps, as there
        for fs in ("2.6e+06", "1e+07", "2.5e+07", "2.09715e+06"):
            assert res[f"timeline@{fs}", ms].maps > 0.6 * 0.8 * 240


# ---- 5. the timelines' own records ------------------------------------------------------------------------------------------------------
def test_every_engineered_event_sits_on_its_block():
    kinds = set()
    for name, cin, record, fs, nsamp in edge_timelines():
        A.check_record(cin, record, fs)
        kinds |= {e["kind"] for e in record}
        assert np.all(np.abs(cin["f_carr"] * (1.0 / fs)) < 0.5) and cin.shape[1] == A.NC
        for nchan in (1, 5, 16):                                      # ... and in every column group a case with fewer channels runs
            ps = A.parts(cin, record, nchan)
            assert sum(len(r) for _, r in ps) == len(record) and sum(c.shape[1] for c, _ in ps) == A.NC
            for c, r in ps:
                A.check_record(c, r, fs)
    assert kinds == {"change", "unused_begins", "unused_ends", "doppler_zero", "doppler_sign", "unused_wave", "unused_wave_back", "unused_round",
                     "unused_round_back", "unused_round_end", "unused_final", "never_used", "unused_before", "addend_not_walked_before",
                     "stretch_mix", "table_threshold", "tie"}
    # the scan positions and the workgroup edges, from the kernels' constants
    assert A.SCAN_POSITIONS == (63, 64, 1023, 1024, 2047, 2048)
    assert [A.K_LANE_THREADS // k for k in (4, 8, 16, 32)] == [64, 32, 16, 8]
    assert [A.lanes_per_block(m) for m in (1, 2, 4, 5, 8, 9, 16, 17, 31, 32)] == [4, 4, 4, 8, 8, 16, 16, 32, 32, 32]
    big, rec = A.scan_edge_timeline(2049)
    on = {(e["kind"], e["block"]) for e in rec}
    for kind in ("change", "unused_begins", "unused_ends"):
        assert {p for k, p in on if k == kind} == set(A.SCAN_POSITIONS), kind
    assert {p for k, p in on if k in ("doppler_zero", "doppler_sign")} == set(A.SCAN_POSITIONS)
