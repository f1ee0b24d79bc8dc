"""gpsiq_stap_beams on the MI355X: every output byte, every guard byte around every destination and every count equals
tests/_stap_beams_ref.py's restatement of the contract (include/gpsiq_rows.h, "Space-time array", "Several beams from one pass"), on
each kernel that can serve -- stap_beams_generic and stap_beams_mfma<IN, OUT, TP>, all four format pairs -- forced through
GPSIQ_STAP_BEAMS_KERNEL and confirmed with gpsiq_stap_beams_last_plan against the planner (tests/stap_beams_plan.cpp).  Where the
matrix kernel cannot serve (a shape that does not pad into 32 rows, a weight outside the digit planes) the forced call falls to the
generic kernel, and that fall is confirmed the same way.  The shapes are the smallest at which a kernel can go wrong; the numbers of
the edges are the planner's.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import _stap_beams_plan as bp
import _stap_beams_ref as br
import _stap_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
PAD = 64
AT = 8                                  # where a case's span starts in the pool: the samples before it are its heads
SHAPES = [(1, 1), (1, 8), (2, 4), (4, 2), (8, 1), (3, 3), (4, 5), (5, 5), (8, 4), (4, 8)]       # tests/test_gpu_stap.py's list
BEAMS = (1, 2, 3, 7, 8)
KERNELS = ("generic", "mfma")
PAIRS = pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)], ids=["8to8", "8to16", "16to8", "16to16"])


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def pool(size, kind="random"):
    """eight streams of a format every case cuts its elements and their heads from (computed once, never written)"""
    p = sr.streams(np.random.default_rng(6100 + size + len(kind)), 8, 12000, size, kind)
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def cut(size, nelem, ntaps, at, nsamp, heads="all", kind="random"):
    p = pool(size, kind)[:nelem]
    xs = [x[at:at + nsamp] for x in p]
    hs = sr.heads_of(p, at, ntaps)
    return xs, None if heads == "none" else hs if heads == "all" else [h if e % 2 == 0 else None for e, h in enumerate(hs)]


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_STAP_BEAMS_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_STAP_BEAMS_KERNEL", kernel)


def upload(arrays, offset=0):
    """the arrays in ONE device buffer, each at a 16-byte aligned address plus `offset` bytes (a multiple of 4); None stays a null
    pointer -> (buffer, pointers)"""
    import torch
    assert offset % 4 == 0
    sizes = [0 if a is None else np.asarray(a).nbytes for a in arrays]
    stride = [(-(-(s + offset) // 16) + 1) * 16 for s in sizes]
    raw = np.full(sum(stride) + 16, GUARD, np.uint8)
    at, ptrs = 0, []
    for a, s, st in zip(arrays, sizes, stride):
        if a is not None:
            raw[at + offset:at + offset + s] = np.ascontiguousarray(a).view(np.uint8).ravel()
        ptrs.append(None if a is None else at + offset)
        at += st
    buf = torch.from_numpy(raw).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, [0 if p is None else buf.data_ptr() + p for p in ptrs]


def planned(nelem, ntaps, nbeams, nsamp, in_size, out_size, w, kernel):
    return bp.ask([("plan", nelem, ntaps, nbeams, nsamp, in_size, out_size, br.max_entry(w), bp.FORCE[kernel])])[0]


def run_beams(ctx, kernel, xs, heads, w, shift, out_size, dst_offsets=(0, 4, 8, 12), offset=0, head_offset=0):
    """one call with every destination in ONE guarded buffer, destination b at 16-byte alignment plus dst_offsets[b % 4] -> (outputs,
    counts); the guards and the plan are checked here"""
    import torch
    w = np.asarray(w)
    in_size, nsamp, nbeams = np.asarray(xs[0]).dtype.itemsize, len(xs[0]), w.shape[0]
    buf, ptrs = upload(xs, offset)
    hbuf, hptrs = (None, None) if heads is None else upload(heads, head_offset)
    olen = 2 * nsamp * out_size
    stride = 2 * PAD + -(-olen // 16) * 16 + 16
    dst = torch.full((nbeams * stride,), GUARD, dtype=torch.uint8, device="cuda")
    ats = [b * stride + PAD + dst_offsets[b % len(dst_offsets)] for b in range(nbeams)]
    counts, ms = ctx.stap_beams(ptrs, nsamp, in_size, w, shift, out_size, [dst.data_ptr() + a for a in ats], heads=hptrs)
    got = dst.cpu().numpy()
    assert ms >= 0.0 and counts.dtype == np.uint64 and counts.shape == (nbeams,)
    guard = np.ones(len(got), bool)
    for a in ats:
        guard[a:a + olen] = False
    assert (got[guard] == GUARD).all(), "guard bytes around a destination changed"
    plan = planned(len(xs), w.shape[2], nbeams, nsamp, in_size, out_size, w, kernel)
    last = ctx.stap_beams_last_plan()
    assert last[3:6] == (len(xs), w.shape[2], nbeams)
    if plan is None:
        assert last[0] is None
    else:
        assert (last[0], last[1], last[2], last[6]) == (bp.KERNELS[plan.kernel], plan.grid, plan.run, plan.padded)
        if kernel == "generic" or (kernel == "mfma" and plan.can):
            assert last[0] == kernel
    del buf, hbuf
    dtype = np.int8 if out_size == 1 else np.int16
    return [got[a:a + olen].view(dtype).reshape(-1, 2).copy() for a in ats], counts


def check_beams(ctx, monkeypatch, xs, heads, w, shift, out_size, kernels=KERNELS, **kw):
    """every kernel that can be asked for against the restatement, computed once -> the counts"""
    want, wc = br.beams_ref(xs, heads, w, shift, out_size)
    for kernel in kernels:
        set_kernel(monkeypatch, kernel)
        got, gc = run_beams(ctx, kernel, xs, heads, w, shift, out_size, **kw)
        for b, (g, y) in enumerate(zip(got, want)):
            bad = np.flatnonzero((g != y).any(axis=1))
            assert not len(bad), (kernel, len(xs), np.asarray(w).shape, len(xs[0]), shift, out_size, kw, "beam", b, "first differing sample", int(bad[0]),
                                  g[bad[0]].tolist(), y[bad[0]].tolist())
        assert np.array_equal(gc, wc), (kernel, gc.tolist(), wc.tolist())
    return wc


def random_weights(rng, nbeams, nelem, ntaps, shift):
    rows = nelem * ntaps
    lim = min(65535 // (2 * rows), br.MAX_ENTRY) if shift else 3         # shift 0: small weights, so that not everything is clamped
    return rng.integers(-lim, lim + 1, size=(nbeams, nelem, ntaps, 2)).astype(np.int16)


@pytest.mark.parametrize("nelem,ntaps", SHAPES)
@PAIRS
def test_every_edge_on_every_kernel(ctx, monkeypatch, in_size, out_size, nelem, ntaps):
    """nsamp 0, 1, ntaps - 1, either side of an instruction's 16 columns, of a wave's tile, of a workgroup's run of either kernel and
    several runs with a ragged tail; 1, 2, 3, 7 and 8 beams, heads for all, none and some, and every alignment of sources, heads and
    destinations in turn -- the destinations of one call each at its own"""
    lim = bp.limits()
    tile = lim.tile8 if out_size == 1 else lim.tile16
    runs = sorted({planned(nelem, ntaps, 2, 100, in_size, out_size, np.zeros((1, 1, 1, 2), np.int16), k).run for k in KERNELS})
    sizes = [0, 1, ntaps - 1, 15, 16, 17, tile - 1, tile + 1] + [r + d for r in runs for d in (-1, 0, 1)] + [3 * runs[-1] + 2 * tile + 5]
    rng = np.random.default_rng(190 + 10 * in_size + out_size + nelem + ntaps)
    for i, nsamp in enumerate(sizes):
        xs, heads = cut(in_size, nelem, ntaps, AT + 2 * i, nsamp, ("all", "none", "some")[i % 3])
        shift = (0, 14, 24)[i % 3] if in_size == 2 else (0, 7, 16)[i % 3]
        w = random_weights(rng, BEAMS[i % len(BEAMS)], nelem, ntaps, shift)
        off = (0, 4, 8, 12)
        check_beams(ctx, monkeypatch, xs, heads, w, shift, out_size, dst_offsets=off[i % 4:] + off[:i % 4], offset=off[(i // 2) % 4], head_offset=off[(i + 1) % 4])
    assert ctx.stap_beams_last_plan()[0] == ("generic" if bp.padded_taps(nelem, ntaps) == 0 else "mfma")       # (5, 5) does not pad: the fall


@pytest.mark.parametrize("nelem,ntaps", [(1, 1), (1, 8), (2, 4), (8, 4), (4, 5)])
def test_weights_at_the_bound_against_the_extremes(ctx, monkeypatch, nelem, ntaps):
    """four beams, one per pair of signs, every input at the format's minimum, heads too: |acc| reaches 65535 * 128 and 65535 * 32768 in
    both signs on both components -- where a plane recombination or a row constant that is off wraps.  One row holds the bound only
    with a weight outside the digit planes: that shape is the generic kernel's, and the planner says so."""
    w = np.stack([br.weights_at_the_bound(nelem, ntaps, s) for s in ((1, 1), (1, -1), (-1, 1), (-1, -1))])
    clipped = 0
    for in_size in (SC08, SC16):
        lo, dtype = (-128, np.int8) if in_size == 1 else (-32768, np.int16)
        worst = [np.full((777, 2), lo, dtype) for _ in range(nelem)]
        worst_heads = [np.full((ntaps - 1, 2), lo, dtype) for _ in range(nelem)]
        for out_size, shift in ((SC08, 24), (SC16, 14), (SC16, 0)):
            clipped += int(check_beams(ctx, monkeypatch, worst, worst_heads, w, shift, out_size).sum())
            xs, heads = cut(in_size, nelem, ntaps, AT, 777, kind="extremes")
            clipped += int(check_beams(ctx, monkeypatch, xs, heads, w, shift, out_size, dst_offsets=(4, 12, 0, 8)).sum())
    assert clipped > 0
    assert (ctx.stap_beams_last_plan()[0] == "mfma") == (nelem * ntaps > 1)


@pytest.mark.parametrize("nelem,ntaps", [(3, 3), (4, 5), (1, 8), (2, 4)])
def test_zero_samples_of_int16_input_show_in_every_bit(ctx, monkeypatch, nelem, ntaps):
    """no heads, padded taps, shift 0, int16 output: the samples before the span are the pair (lo' = -128, hi = 0) in the matrix
    kernel's planes, and the row constant has to cancel them to the last bit; spans shorter than the taps among them"""
    rng = np.random.default_rng(5 + nelem)
    for nsamp, nbeams in ((1, 8), (ntaps - 1, 3), (ntaps + 1, 2), (300, 7)):
        xs, _ = cut(SC16, nelem, ntaps, AT, nsamp, "none")
        w = rng.integers(-1, 2, size=(nbeams, nelem, ntaps, 2)).astype(np.int16)
        check_beams(ctx, monkeypatch, xs, None, w, 0, SC16)
        small = [(x // 64).astype(np.int16) for x in xs]               # |x| <= 512: at most 40 terms of it, nothing is clamped
        assert check_beams(ctx, monkeypatch, small, [None] * nelem, w, 0, SC16).sum() == 0


@PAIRS
def test_a_weight_just_inside_and_just_outside_the_digit_planes(ctx, monkeypatch, in_size, out_size):
    xs, heads = cut(in_size, 2, 2, AT, 1500, kind="extremes")
    shift = 13 if in_size == 1 else 21
    for entry, serves in (((32639, 0), True), ((32640, 0), False), ((0, 32639), True), ((0, 32640), False), ((0, -32639), True), ((5, -32768), False),
                          ((-32768, 0), True)):
        w = np.random.default_rng(abs(entry[0]) + abs(entry[1])).integers(-900, 901, size=(3, 2, 2, 2)).astype(np.int16)
        w[1, 1, 0] = entry
        assert (br.max_entry(w) <= br.MAX_ENTRY) == serves
        check_beams(ctx, monkeypatch, xs, heads, w, shift, out_size)
        assert ctx.stap_beams_last_plan()[0] == ("mfma" if serves else "generic")      # the last call was forced to the matrix kernel


@PAIRS
def test_a_beam_that_clamps_everywhere_beside_one_that_never_does(ctx, monkeypatch, in_size, out_size):
    """loud beams 0, 3 and 6 among eight: beams 0 and 1 are adjacent accumulator rows of one lane, 3 sits beside 2 in the next row
    group, 6 and 7 in the last"""
    lo, dtype = (-128, np.int8) if in_size == 1 else (-32768, np.int16)
    nelem, ntaps, nsamp = 2, 4, 1111
    xs = [np.full((nsamp, 2), lo, dtype) for _ in range(nelem)]
    heads = [np.full((ntaps - 1, 2), lo, dtype) for _ in range(nelem)]
    w = np.zeros((8, nelem, ntaps, 2), np.int16)
    for b in (0, 3, 6):
        w[b, :, :, 0] = 65535 // 8
        w[b, 0, 0, 0] += 7
    counts = check_beams(ctx, monkeypatch, xs, heads, w, 0, out_size)
    assert counts.tolist() == [2 * nsamp if b in (0, 3, 6) else 0 for b in range(8)]


# ---- identities against the device's own earlier stages ------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@PAIRS
def test_every_beam_is_the_devices_own_combiner(ctx, monkeypatch, kernel, in_size, out_size):
    import torch
    set_kernel(monkeypatch, kernel)
    rng = np.random.default_rng(41)
    for nelem, ntaps, nbeams in ((2, 4, 8), (3, 3, 3), (4, 8, 2)):
        nsamp = 4001
        xs, heads = cut(in_size, nelem, ntaps, AT, nsamp, "some", kind="extremes")
        shift = 12 if in_size == 1 else 20
        w = random_weights(rng, nbeams, nelem, ntaps, shift)
        got, counts = run_beams(ctx, kernel, xs, heads, w, shift, out_size)
        buf, ptrs = upload(xs)
        hbuf, hptrs = upload(heads)
        for b in range(nbeams):
            y = torch.zeros(2 * nsamp * out_size, dtype=torch.uint8, device="cuda")
            c, _ = ctx.stap_combine(ptrs, nsamp, in_size, w[b], shift, out_size, y.data_ptr(), heads=hptrs)
            assert np.array_equal(y.cpu().numpy(), got[b].view(np.uint8).ravel()) and c == counts[b], (nelem, ntaps, b)
        del buf, hbuf


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_tap_is_the_array_combiner_and_one_element_one_beam_the_complex_filter(ctx, monkeypatch, kernel):
    import torch
    set_kernel(monkeypatch, kernel)
    rng = np.random.default_rng(43)
    for in_size, out_size, shift in ((SC08, SC16, 9), (SC16, SC08, 21)):
        nsamp = 3001
        xs, _ = cut(in_size, 4, 1, AT, nsamp, kind="extremes")
        w = random_weights(rng, 3, 4, 1, shift)
        got, counts = run_beams(ctx, kernel, xs, None, w, shift, out_size)
        buf, ptrs = upload(xs)
        for b in range(3):
            y = torch.zeros(2 * nsamp * out_size, dtype=torch.uint8, device="cuda")
            c, _ = ctx.array_combine(ptrs, nsamp, in_size, w[b, :, 0], shift, out_size, y.data_ptr())
            assert np.array_equal(y.cpu().numpy(), got[b].view(np.uint8).ravel()) and c == counts[b]
        del buf
        for ntaps in (1, 5, 8):
            xs, heads = cut(in_size, 1, ntaps, AT, nsamp, kind="extremes")
            taps = random_weights(rng, 1, 1, ntaps, shift)
            (got1,), (c1,) = run_beams(ctx, kernel, xs, heads, taps, shift, out_size)
            src, (sp_,) = upload(xs)
            hbuf, hp = (None, [0]) if ntaps == 1 else upload(heads)
            y = torch.zeros(2 * nsamp * out_size, dtype=torch.uint8, device="cuda")
            nout, fc, _ = ctx.cfilter(nsamp, in_size, sp_, taps[0, 0], shift, 1, 0, out_size, y.data_ptr(), head_ptr=hp[0] or None)
            assert nout == nsamp and np.array_equal(y.cpu().numpy(), got1.view(np.uint8).ravel()) and fc == c1
            del src, hbuf


# ---- pieces and repeats ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("in_size", [SC08, SC16], ids=["int8", "int16"])
def test_a_span_in_pieces_is_one_call_and_a_call_repeats(ctx, monkeypatch, kernel, in_size):
    """three pieces, the second shorter than ntaps - 1; every piece's head is the last ntaps - 1 samples before it"""
    set_kernel(monkeypatch, kernel)
    nelem, ntaps, nbeams, nsamp = 3, 6, 5, 5000
    out_size, shift = SC08, 9 if in_size == 1 else 17
    w = np.random.default_rng(3).integers(-900, 901, size=(nbeams, nelem, ntaps, 2)).astype(np.int16)
    xs, heads = cut(in_size, nelem, ntaps, AT, nsamp)
    want, wc = br.beams_ref(xs, heads, w, shift, out_size)
    assert (wc > 0).all()
    whole, count = run_beams(ctx, kernel, xs, heads, w, shift, out_size)
    again, count2 = run_beams(ctx, kernel, xs, heads, w, shift, out_size)
    assert all(np.array_equal(a, b) and np.array_equal(a, y) for a, b, y in zip(whole, again, want)) and np.array_equal(count, count2) and np.array_equal(count, wc)
    cuts = [0, 2051, 2054, nsamp]
    pieces, total = [[] for _ in range(nbeams)], np.zeros(nbeams, np.uint64)
    for lo, hi in zip(cuts, cuts[1:]):
        pxs, ph = cut(in_size, nelem, ntaps, AT + lo, hi - lo)
        ys, c = run_beams(ctx, kernel, pxs, ph, w, shift, out_size, offset=(0, 4, 8, 12)[lo % 4], dst_offsets=(8, 0, 12, 4))
        for b in range(nbeams):
            pieces[b].append(ys[b])
        total += c
    assert all(np.array_equal(np.concatenate(p), y) for p, y in zip(pieces, want)) and np.array_equal(total, wc)


@pytest.mark.parametrize("in_size", [SC08, SC16], ids=["int8", "int16"])
def test_the_planner_chooses_what_it_says(ctx, monkeypatch, in_size):
    """either side of every threshold of the default, and shapes the matrix kernel cannot serve"""
    for nelem, ntaps, nbeams in ((1, 1, 1), (2, 4, 3), (2, 4, 4), (4, 4, 4), (4, 4, 7), (1, 1, 8), (1, 2, 8), (1, 8, 8), (2, 2, 4), (8, 4, 8), (5, 5, 8)):
        xs, heads = cut(in_size, nelem, ntaps, AT, 3000)
        w = random_weights(np.random.default_rng(nbeams), nbeams, nelem, ntaps, 12)
        check_beams(ctx, monkeypatch, xs, heads, w, 12 if in_size == 1 else 20, SC08, kernels=(None,))
        tp = bp.padded_taps(nelem, ntaps)
        assert ctx.stap_beams_last_plan()[0] == ("mfma" if tp and bp.default_is_mfma(in_size, nelem * tp, nbeams) else "generic")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import torch
    x = [torch.zeros(4096, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ptrs = [t.data_ptr() for t in x]
    hd = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    d = dst.data_ptr()

    def wk(nbeams, nelem=2, ntaps=2):
        w = np.zeros((nbeams, nelem, ntaps, 2), np.int16)
        w[:, 0, 0, 0] = 1
        return w

    def code(call):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call()
        return e.value.code

    e_arg = code(lambda: ctx.stap_beams(ptrs, -1, SC08, wk(1), 0, SC08, [d]))
    over = wk(2)
    over[1, 0, 0], over[1, 1, 0] = (32767, 0), (32767, 2)               # beam 0 legal, beam 1 over the bound by one
    e_range = code(lambda: ctx.stap_beams(ptrs, 100, SC08, over, 0, SC08, [d, d + 1024]))
    assert e_arg != e_range
    over[1, 1, 0] = (32767, 1)                                           # the bound itself
    assert ctx.stap_beams(ptrs, 100, SC08, over, 0, SC08, [d, d + 1024])[0].tolist() == [0, 0]
    bad = [lambda: ctx.stap_beams(ptrs, 10, SC08, wk(0), 0, SC08, []),                                          # no beam
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(9), 0, SC08, [d + 64 * b for b in range(9)]),               # nine beams
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), 0, SC08, [d, 0]),                                       # a null destination
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), 0, SC08, [d, d + 1026]),                                # a misaligned one
           lambda: ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d, d + 196]),                                # destinations that overlap by one dword
           lambda: ctx.stap_beams(ptrs, 100, SC08, wk(3), 0, SC08, [d, d + 1024, d]),                            # the same destination twice
           lambda: ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d, ptrs[1] + 196]),                          # over a source's last dword
           lambda: ctx.stap_beams([ptrs[0], ptrs[0] + 400], 100, SC08, wk(2), 0, SC16, [d, ptrs[0] + 4]),        # a wider output reaching into one
           lambda: ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d, d + 1024], heads=[0, d + 1024]),          # over a head
           lambda: ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d, d + 1024], heads=[d + 196, 0]),
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), 0, 3, [d, d + 1024]), lambda: ctx.stap_beams(ptrs, 10, 4, wk(2), 0, SC08, [d, d + 1024]),     # formats
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), -1, SC08, [d, d + 1024]), lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), 25, SC08, [d, d + 1024]),   # shift
           lambda: ctx.stap_beams([ptrs[0], 0], 10, SC08, wk(2), 0, SC08, [d, d + 1024]),                        # a null source
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(2), 0, SC08, [d, d + 1024], heads=[hd.data_ptr() + 2, 0]),  # a misaligned head
           lambda: ctx.stap_beams(ptrs, 10, SC08, wk(1, 2, 9), 0, SC08, [d])]                                    # nine taps
    for k, call in enumerate(bad):
        assert code(call) == e_arg, k
    # a null pointer is no fault where there is nothing to read or write, and the counts are written: zeros
    assert ctx.stap_beams([0, 0], 0, SC08, wk(3), 0, SC08, [0, 0, 0])[0].tolist() == [0, 0, 0] and ctx.stap_beams_last_plan()[0] is None
    # side by side is no overlap
    assert ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d, d + 200])[0].tolist() == [0, 0]
    assert ctx.stap_beams(ptrs, 100, SC08, wk(2), 0, SC08, [d + 4, d + 204], heads=[d, d + 404])[0].tolist() == [0, 0]
