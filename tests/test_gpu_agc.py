"""gpsiq_agc on the MI355X: every output byte, every guard byte, both counts, every multiplier and the returned state equal
tests/_agc_ref.py's restatement of the contract (include/gpsiq_rows.h, "AGC"), in all four format pairs.  The spans are random
full-range elements unless a case says otherwise, every source ends in poison bytes and every destination lies between guard bytes of
0x7f that must not change.  The shapes are the smallest at which a kernel can go wrong: both sides of a wave, of a tile of agc_measure
and of a workgroup of agc_apply (from the plan query), windows that begin anywhere in a unit, rings that come from the state, from the
span and from both, every hold around a unit and a wave, exceeding samples on the edges of lanes, tiles and the span.
Run with -m gpu."""
import numpy as np
import pytest

import _agc_plan as ap
import _agc_ref as ar
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
POISON = 0xA5                    # behind every source: 0xA5A5 as a sample would not go unnoticed
PAD = 64                         # guard bytes either side of a destination
PAIRS = pytest.mark.parametrize("in_size,out_size", [(SC08, SC08), (SC08, SC16), (SC16, SC08), (SC16, SC16)], ids=["8to8", "8to16", "16to8", "16to16"])
HOLDS = (0, 1, 63, 64, 65, 1024)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """full-range samples of either format every case cuts its span from (computed once, never written)"""
    rng = np.random.default_rng(91)
    p = {ss: ar.full_range(rng, 40000, ss) for ss in (SC08, SC16)}
    for a in p.values():
        a.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def limits():
    return ap.limits()


def qmax_of(out_size):
    return 127 if out_size == SC08 else 32767


def target_for(in_size, out_size):
    """a target at which a full-range random span (uniform: its peak is 1.73 times its rms) clips some elements and not most"""
    return 256 * (100 if out_size == SC08 else 25000)


def thresh_for(in_size):
    """full-range elements exceed it now and then: about one sample in eleven"""
    return 122 if in_size == SC08 else 31300


def make_state(rng, c, in_size, fill, nring, hold=0):
    """a state a stream of this format could have left: nring windows, some partly blanked, and `fill` samples of the next"""
    top = (1 << 14) if in_size == SC08 else (1 << 30)
    ring = []
    for _ in range(nring):
        k = 2 * int(rng.integers(0, c.window + 1)) if rng.integers(0, 4) == 0 else 2 * c.window
        ring.append((int(rng.integers(0, k * top // 3 + 1)), k))
    k = 2 * int(rng.integers(0, fill + 1))
    return ar.State(tuple(ring), int(rng.integers(0, k * top // 3 + 1)), k, fill, hold)


def device_bytes(a, skew):
    """the bytes of array a on the device, `skew` bytes past a 16-byte boundary, poison before and behind -> (tensor, pointer)"""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).ravel()
    raw = np.full(16 + len(b) + 64, POISON, np.uint8)
    raw[skew:skew + len(b)] = b
    t = torch.from_numpy(raw).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + skew


def run_agc(ctx, x, c, state, out_size, skew=(0, 0)):
    """x [n, 2] -> (out [n, 2] as the device wrote it, clipped, blanked, mults, the state returned); guards compared.  skew: bytes the
    span and the destination start past a 16-byte boundary"""
    import torch
    n = len(x)
    src, src_ptr = device_bytes(x, skew[0])
    olen = 2 * n * out_size
    dst = torch.full((2 * PAD + 16 + olen,), GUARD, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    lead = PAD + skew[1]
    st = ar.to_lib_state(state)
    clipped, blanked, mults, ms = ctx.agc(n, x.dtype.itemsize, src_ptr, ar.to_lib_cfg(c), out_size, dst.data_ptr() + lead, state=st)
    got = dst.cpu().numpy()
    assert ms >= 0.0
    assert (got[:lead] == GUARD).all() and (got[lead + olen:] == GUARD).all(), "guard bytes of the destination changed"
    del src
    out = got[lead:lead + olen].copy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2)
    return out, clipped, blanked, mults.tolist(), ar.from_lib_state(st)


def check(ctx, x, c, state, out_size, skew=(0, 0)):
    want = ar.agc_ref(x, c, state, out_size)
    got = run_agc(ctx, x, c, state, out_size, skew)
    what = (len(x), c, state.fill, len(state.ring), state.hold)
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert not len(bad), (what, "first differing sample", int(bad[0]), got[0][bad[0]], want[0][bad[0]])
    assert got[3] == want[3], (what, "multipliers")
    assert got[1] == want[1] and got[2] == want[2], (what, "clipped, blanked", got[1:3], want[1:3])
    assert got[4] == want[4], (what, "state", got[4], want[4])
    return want


@PAIRS
def test_span_lengths_windows_rings_and_fills(ctx, pool, limits, in_size, out_size):
    """nsamp either side of a unit, a wave's window, a tile and a workgroup; window 64 and 128; navg 1, 2 and 64 -- more than the span
    completes --; an incoming fill of 0, 1 and W - 1 with a ring of 0, 1 and navg windows from the state; the blanker on, the hold walking
    through its edges"""
    rng = np.random.default_rng(100 + 10 * in_size + out_size)
    sizes = [1, 63, 64, 65, 127, 128, 129, limits.tile - 1, limits.tile, limits.tile + 1, limits.apply_tile - 1, limits.apply_tile, limits.apply_tile + 1]
    i = 0
    seen = set()
    for nsamp in sizes:
        for W in (64, 128):
            for navg in (1, 2, 64):
                for fill in (0, 1, W - 1):
                    H = HOLDS[i % len(HOLDS)]
                    c = ar.cfg(window=W, navg=navg, target_q8=target_for(in_size, out_size), mult0=3000 + i, blank_thresh=thresh_for(in_size), blank_hold=H,
                               qmax=qmax_of(out_size))
                    nring = (0, 1, navg)[(i // 3) % 3]
                    st = make_state(rng, c, in_size, fill, nring, hold=(0, H, H // 2)[i % 3])
                    x = pool[in_size][i:i + nsamp]
                    want = check(ctx, x, c, st, out_size)
                    seen.add((want[1] > 0, want[2] > 0, len(want[3]) > navg))
                    if nsamp in (limits.tile, limits.apply_tile + 1):
                        p = ap.plan(nsamp, W, fill, True)
                        assert ctx.agc_last_plan() == (p.measure, limits.tile, p.gains, p.apply, limits.apply_tile, 0)
                    i += 1
    # (int8 into int16 cannot clip below the largest multiplier: 128 * 2^24 / 65536 is the clamp itself)
    assert (in_size, out_size) == (SC08, SC16) or {s[0] for s in seen} == {True, False}
    assert {s[1] for s in seen} == {True, False} and {s[2] for s in seen} == {True, False}


@pytest.mark.parametrize("in_size", [SC08, SC16], ids=["int8", "int16"])
@pytest.mark.parametrize("H", HOLDS)
def test_every_hold_with_exceeding_samples_on_the_edges(ctx, pool, limits, in_size, H):
    """a quiet span (a quarter of the range) with exceeding samples on the last lane of a wave, the last sample of a tile, the first and
    the last sample of the span, H + 1 apart (one unblanked sample between two holds), H apart, and across a tile's edge; three tiles and
    a ragged end, so that a lead-in of 1024 samples reaches back over half a tile"""
    tile = limits.tile
    nsamp = 3 * tile + 77
    x = (pool[in_size][:nsamp] // 4).copy()
    big = np.array([-128, 127] if in_size == SC08 else [-32768, 32767], x.dtype)
    wave = 64 * limits.unit
    spots = [0, wave - 1, 2 * wave - 1, tile - 1, tile, 2 * tile - 1, nsamp - 1, 700, 700 + H + 1, 2500, 2500 + H, 2 * tile - 3, 2 * tile + H - 2,
             2 * tile + 2 * H + 40]
    for k, at in enumerate(spots):
        if 0 <= at < nsamp:
            x[at, k % 2] = big[(k // 2) % 2]
    thresh = 100 if in_size == SC08 else 20000
    c = ar.cfg(window=192, navg=3, target_q8=256 * 40, mult0=65536, blank_thresh=thresh, blank_hold=H, qmax=127)
    want = check(ctx, x, c, ar.FRESH, SC08)
    assert want[2] >= len(set(spots)) and want[4].hold == H           # the last sample exceeds: the whole hold is left
    # the same with the span ending on, H - 1 and H samples behind its last exceeding sample
    for cut in sorted({1, H, H + 1} - {0}):
        y = np.concatenate([x, x[5:5 + cut - 1] // 2])
        want = check(ctx, y, c, ar.FRESH, SC08)
        assert want[4].hold == max(0, H - (len(y) - nsamp))


def test_hold_edges(ctx, pool):
    # a span shorter than the incoming hold: every sample blanked, the rest of the hold handed on, no power, no clip
    c = ar.cfg(window=64, navg=2, target_q8=256 * 60, mult0=5000, blank_thresh=120, blank_hold=9, qmax=127)
    want = check(ctx, pool[SC08][:5] // 4, c, ar.State((), 0, 0, 3, 9), SC08)
    assert want[2] == 5 and want[4].hold == 4 and want[4].pcnt == 0 and (want[0] == 0).all()
    # the blanker off and a hold handed in all the same (blank_hold may be set with the threshold at 0): no mask, the hold still counts
    c0 = c._replace(blank_thresh=0)
    want = check(ctx, pool[SC08][:300], c0, ar.State((), 0, 0, 3, 9), SC08)
    assert want[2] == 9 and want[4].hold == 0
    assert check(ctx, pool[SC08][:4], c0, ar.State((), 0, 0, 3, 9), SC08)[4].hold == 5
    # a window blanked whole: its count is 0, and with navg 1 the window behind it has n = 0 and takes mult0
    x = (pool[SC16][:64 * 8] // 8).copy()
    x[64, 0] = 30000
    c = ar.cfg(window=64, navg=1, target_q8=256 * 1000, mult0=7777, blank_thresh=20000, blank_hold=150, qmax=32767)
    want = check(ctx, x, c, ar.FRESH, SC16)
    assert want[3][0] == 7777 and want[3][3] == 7777 and want[3][4] != 7777 and 7777 not in want[3][5:] and want[2] == 151
    # a threshold of 32767: only -32768 exceeds it; an int8 stream never does
    x = pool[SC16][:3000].copy()
    x[x == -32768] = -32767
    x[1000, 1] = -32768
    x[2000, 0] = 32767
    c = ar.cfg(window=128, navg=4, target_q8=256 * 9000, blank_thresh=32767, blank_hold=10, qmax=32767)
    assert check(ctx, x, c, ar.FRESH, SC16)[2] == 11
    x8 = pool[SC08][:3000]
    assert check(ctx, x8, c, ar.FRESH, SC16)[2] == 0 and check(ctx, x8, c._replace(blank_thresh=127, qmax=127), ar.FRESH, SC08)[2] > 0


@PAIRS
def test_extreme_elements_clamps_and_qmax(ctx, pool, in_size, out_size):
    dt = np.int8 if in_size == SC08 else np.int16
    lo = -128 if in_size == SC08 else -32768
    n = 1000
    # an all-zero span: S = 0, r clamped to 1, the multiplier at its upper clamp; nothing to clip
    c = ar.cfg(window=128, navg=2, target_q8=256 * 50, mult0=65536, mult_max=(1 << 24) - 1, qmax=qmax_of(out_size))
    want = check(ctx, np.zeros((n, 2), dt), c, ar.FRESH, out_size)
    assert want[3][1] == min((256 * 50) << 16, (1 << 24) - 1) and want[1] == 0
    # a span of the most negative value: S = n * 2^30 for int16, the largest a ring can hold with navg 64 windows of it behind
    st = ar.State(tuple((128 * 2 * lo * lo, 256) for _ in range(64)), 0, 0, 0, 0)
    c = ar.cfg(window=128, navg=64, target_q8=256 * 100, mult0=65536, qmax=qmax_of(out_size))
    want = check(ctx, np.full((n, 2), lo, dt), c, st, out_size)
    assert want[3][0] == ((256 * 100) << 16) // (-lo * 256) and (want[0] == want[0][0, 0]).all()
    # both multiplier clamps biting: a loud window drives the rule below mult_min, a quiet one above mult_max
    x = pool[in_size][:n].copy()
    x[256:512] //= 64 if in_size == SC08 else 4096
    c = ar.cfg(window=128, navg=1, target_q8=256 * 20, mult0=40000, mult_min=39000, mult_max=41000, qmax=qmax_of(out_size))
    want = check(ctx, x, c, ar.FRESH, out_size)
    free = ar.agc_ref(x, c._replace(mult_min=1, mult_max=(1 << 24) - 1), ar.FRESH, out_size)[3]
    assert 39000 in want[3] and 41000 in want[3] and min(free) < 39000 and max(free) > 41000
    # every qmax the format can hold
    for q in (1, 7, 127, 32767):
        if q > qmax_of(out_size):
            with pytest.raises(gpsiq.GpsiqError) as e:
                run_agc(ctx, x, c._replace(qmax=q), ar.FRESH, out_size)
            assert e.value.code == -1
            continue
        want = check(ctx, x, c._replace(qmax=q, mult0=65536, mult_min=1, mult_max=(1 << 24) - 1, target_q8=256 * q), ar.FRESH, out_size)
        if q < 32767 or in_size == SC16:                             # (the first window passes the input through: int8 never reaches 32767)
            assert want[1] > 0 and np.abs(want[0].astype(np.int32)).max() == q


def test_exact_counts_at_qmax_by_hand(ctx):
    """mult0 = 65536 passes the input through: values at qmax pass uncounted, one beyond is clamped and counted, blanked ones are neither"""
    x = np.array([[126, 127], [128, -127], [-128, -129], [0, 32767], [500, 3]], np.int16)
    c = ar.cfg(window=64, navg=1, mult0=65536, blank_thresh=400, blank_hold=0, qmax=127)
    out, clipped, blanked, mults, st = run_agc(ctx, x, c, ar.FRESH, SC08)
    assert out.tolist() == [[126, 127], [127, -127], [-127, -127], [0, 0], [0, 0]] and clipped == 3 and blanked == 2 and mults == [65536]
    assert st == ar.State((), 126 ** 2 + 127 ** 2 + 128 ** 2 + 127 ** 2 + 128 ** 2 + 129 ** 2, 6, 5, 0)
    # rounding: y = floor((x * mult + 32768) / 65536), also for negative products: -3 * 32768 -> -1.5 -> floor(-1.5 + 0.5) = -1
    x = np.array([[3, -3], [1, -1], [5, -5]], np.int8)
    out = run_agc(ctx, x, c._replace(mult0=32768), ar.FRESH, SC16)[0]
    assert out.tolist() == [[2, -1], [1, 0], [3, -2]]


@pytest.mark.parametrize("in_size", [SC08, SC16], ids=["int8", "int16"])
def test_every_alignment_of_source_and_destination(ctx, pool, in_size):
    """each of the two at 0, 4, 8 and 12 bytes past a 16-byte boundary; poison behind the source, guards around the destination"""
    c = ar.cfg(window=64, navg=2, target_q8=256 * 60, blank_thresh=thresh_for(in_size), blank_hold=5, qmax=127)
    i = 0
    for s in (0, 4, 8, 12):
        for d in (0, 4, 8, 12):
            out_size = (SC08, SC16)[i % 2]
            check(ctx, pool[in_size][77:77 + 1333 + i], c._replace(qmax=qmax_of(out_size), target_q8=target_for(in_size, out_size)), ar.FRESH, out_size, skew=(s, d))
            i += 1


def test_the_same_call_twice(ctx, pool):
    c = ar.cfg(window=128, navg=3, target_q8=256 * 100, blank_thresh=127, blank_hold=20, qmax=127)      # (only -128 exceeds: most samples stay)
    st = ar.State(((1000000, 256),), 1234, 20, 17, 3)
    a = run_agc(ctx, pool[SC08][100:100 + 5000], c, st, SC08, skew=(4, 4))
    b = run_agc(ctx, pool[SC08][100:100 + 5000], c, st, SC08, skew=(4, 4))
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] > 0 and a[2] > 0


@pytest.mark.parametrize("in_size,out_size", [(SC08, SC08), (SC16, SC16), (SC16, SC08)])
def test_pieces_on_the_device_equal_one_call(ctx, pool, limits, in_size, out_size):
    """three splits of one span -- inside a unit, on a window's edge, and pieces shorter than the hold and than a window -- each piece
    called with the state the piece before returned: the bytes, both counts, the concatenated multipliers and the final state of one
    call.  A window continued across a call repeats its multiplier as the next call's mults[0]"""
    import torch
    nsamp = limits.tile + 900
    x = pool[in_size][:nsamp]
    c = ar.cfg(window=192, navg=3, target_q8=target_for(in_size, out_size), mult0=2500, blank_thresh=127 if in_size == SC08 else 32700, blank_hold=65, qmax=qmax_of(out_size))    # (few samples exceed: most stay)
    start = make_state(np.random.default_rng(3), c, in_size, 50, 2, hold=31)
    whole = check(ctx, x, c, start, out_size)
    assert whole[1] > 0 and whole[2] > 0
    odd = 1 if out_size == SC16 else 2                               # (a piece's destination is 4-byte aligned: int8 pieces start on even samples)
    for cuts in ([3 * odd, 1000], [192 - 50, 192 - 50 + 10, 192 - 50 + 40], [limits.tile - odd, limits.tile, limits.tile + 200]):
        edges = [0] + cuts + [nsamp]
        dst = torch.full((2 * nsamp * out_size + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        st, clipped, blanked, mults = ar.to_lib_state(start), 0, 0, []
        for lo, hi in zip(edges, edges[1:]):
            continued = int(st.fill) > 0
            piece, ptr = device_bytes(x[lo:hi], 4)
            cl, bl, mu, _ = ctx.agc(hi - lo, in_size, ptr, ar.to_lib_cfg(c), out_size, dst.data_ptr() + 2 * lo * out_size, state=st)
            mu = mu.tolist()
            assert len(mu) == ar.span(hi - lo, c.window, (50 + lo) % c.window)[0]
            if continued and mults:
                assert mu[0] == mults[-1]
                mu = mu[1:]
            clipped, blanked, mults = clipped + cl, blanked + bl, mults + mu
        got = dst.cpu().numpy()
        assert (got[2 * nsamp * out_size:] == GUARD).all()
        assert np.array_equal(got[:2 * nsamp * out_size].view(whole[0].dtype).reshape(-1, 2), whole[0]), cuts
        assert (clipped, blanked, mults) == whole[1:4] and ar.from_lib_state(st) == whole[4], cuts


def test_refusals_and_an_empty_span(ctx):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    src, dst = buf.data_ptr(), buf.data_ptr() + (1 << 15)
    good = ar.cfg(window=64, navg=2, target_q8=256, mult0=65536, mult_min=10, mult_max=1 << 20, blank_thresh=100, blank_hold=8, qmax=127)

    def call(c=good, st=ar.FRESH, nsamp=100, ss=SC08, src=src, oss=SC08, dst=dst):
        return ctx.agc(nsamp, ss, src, ar.to_lib_cfg(c) if c is not None else None, oss, dst, state=None if st is None else ar.to_lib_state(st))

    def refused(**kw):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == -1, (kw, str(e.value))

    assert len(call()[2]) == 2 and len(call(st=None)[2]) == 2
    # each range limit from both sides
    for ok in (dict(window=65536), dict(navg=1), dict(navg=64), dict(target_q8=1), dict(target_q8=(1 << 23) - 1), dict(mult_min=1), dict(mult_max=(1 << 24) - 1),
               dict(mult0=10), dict(mult0=1 << 20), dict(blank_thresh=0), dict(blank_thresh=32767), dict(blank_hold=0), dict(blank_hold=1024), dict(qmax=1)):
        call(c=good._replace(**ok))
    for bad in (dict(window=0), dict(window=32), dict(window=100), dict(window=65536 + 64), dict(window=-64), dict(navg=0), dict(navg=65), dict(target_q8=0),
                dict(target_q8=1 << 23), dict(mult_min=0), dict(mult_max=1 << 24), dict(mult_min=(1 << 20) + 1), dict(mult0=9), dict(mult0=(1 << 20) + 1),
                dict(blank_thresh=-1), dict(blank_thresh=32768), dict(blank_hold=-1), dict(blank_hold=1025), dict(qmax=0), dict(qmax=128), dict(qmax=-1)):
        refused(c=good._replace(**bad))
    assert len(call(c=good._replace(qmax=32767), oss=SC16)[2]) == 2
    refused(c=good._replace(qmax=32768), oss=SC16)
    refused(c=None)
    for ss in (0, 3, 4):
        refused(ss=ss)
        refused(oss=ss)
    refused(nsamp=-1)
    # a state that cannot have come from a call with this window and navg
    call(st=ar.State(((5, 2), (6, 2)), 9, 2, 63, 8))
    for st in (ar.State(((5, 2), (6, 2), (7, 2)), 0, 0, 0, 0), ar.State((), 0, 0, 64, 0), ar.State((), 9, 4, 1, 0), ar.State((), 0, 0, 0, 9)):
        refused(st=st)
    # pointers: alignment, NULL, overlap
    refused(src=src + 2)
    refused(dst=dst + 2)
    refused(src=None)
    refused(dst=None)
    refused(dst=src + 100)                                           # inside the span's 200 bytes
    refused(dst=src)                                                 # no in-place form
    assert len(call(src=src + 200, dst=src)[2]) == 2                 # the destination's 200 bytes end where the span begins
    refused(src=src + 196, dst=src)
    # no sample: nothing launched, counts of 0, the state unchanged -- also with NULL pointers
    st = ar.to_lib_state(ar.State(((5, 2),), 9, 2, 63, 8))
    before = st.as_tuple()
    cl, bl, mu, ms = ctx.agc(0, SC08, None, ar.to_lib_cfg(good), SC08, None, state=st)
    assert (cl, bl, len(mu), ms) == (0, 0, 0, 0.0) and st.as_tuple() == before and ctx.agc_last_plan()[0] is None
    # NULL multipliers, counts and time are accepted
    cfg = ar.to_lib_cfg(good)
    assert gpsiq._agc(ctx._h, 100, SC08, src, gpsiq.C.byref(cfg), None, SC08, dst, None, None, None, None, None) == 0
