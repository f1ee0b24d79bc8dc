"""gpsiq_stap_cov and gpsiq_stap_combine on the MI355X: every int64 word of the covariance, every output byte, every guard byte and
every count equals tests/_stap_ref.py's restatement of the contract (include/gpsiq_rows.h, "Space-time array"), on every kernel that
can serve -- stap_cov_generic (both formats), stap_cov_mfma<G> (int8, G = 1 .. 4) -- each forced through GPSIQ_STAP_KERNEL and
confirmed with gpsiq_stap_last_plan, whose plan is held to the planner's (tests/stap_plan.cpp).  The shapes are the smallest at which a
kernel can go wrong: every number of row groups, one of them with a ragged last group; both sides of a k-step, of a workgroup's run
and of several; spans shorter than the taps; heads, no heads and some heads; sources at addresses that are 4-byte but not 16-byte
aligned; the extremes of both formats; and the one span at which every wave of the matrix kernel takes a full flush interval plus one
k-step, with and without tiles off the diagonal.  Then the contract's four identities against the device's own gpsiq_array_cov,
gpsiq_array_combine and gpsiq_cfilter, continuation in pieces, and the refusals.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import _stap_plan as sp
import _stap_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
PAD = 64
AT = 8                                  # where a case's span starts in the pool: the samples before it are its heads
# (nelem, ntaps): G = 1; G = 2 (ragged: 9 rows); G = 3 (ragged: 20 rows); G = 4, (5, 5) ragged with 25 rows
SHAPES = [(1, 1), (1, 8), (2, 4), (4, 2), (8, 1), (3, 3), (4, 5), (5, 5), (8, 4), (4, 8)]
SERVING = [("generic", SC08), ("generic", SC16), ("mfma", SC08)]
SERVING_IDS = ["generic-int8", "generic-int16", "mfma-int8"]
FORCE = {"generic": sp.FORCE_GENERIC, "mfma": sp.FORCE_MFMA, None: sp.AUTO}
PAIRS = pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)], ids=["8to8", "8to16", "16to8", "16to16"])


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def lim():
    return sp.limits()


@functools.lru_cache(maxsize=None)
def pool(size, kind="random"):
    """eight streams of a format every case cuts its elements and their heads from (computed once, never written)"""
    p = sr.streams(np.random.default_rng(5100 + size + len(kind)), 8, 20000, size, kind)
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def cut(size, nelem, ntaps, at, nsamp, heads="all", kind="random"):
    """-> (xs, heads): samples [at, at + nsamp) of the pool's first nelem streams and the ntaps - 1 before them: for all, for none
    (None), or for every other element"""
    p = pool(size, kind)[:nelem]
    xs = [x[at:at + nsamp] for x in p]
    hs = sr.heads_of(p, at, ntaps)
    return xs, None if heads == "none" else hs if heads == "all" else [h if e % 2 == 0 else None for e, h in enumerate(hs)]


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_STAP_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_STAP_KERNEL", kernel)


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


def confirm_cov(ctx, kernel, nelem, ntaps, nsamp, in_size):
    plan = sp.ask([("cov", nelem, ntaps, nsamp, in_size, FORCE[kernel])])[0]
    name, grid, run, elements, taps = ctx.stap_last_plan()
    assert (elements, taps) == (nelem, ntaps)
    if plan is None:
        assert name is None
        return
    assert (name, grid, run) == (sp.KERNELS[plan.kernel], plan.grid, plan.run)
    if kernel is not None:
        assert name == kernel


def check_cov(ctx, kernel, xs, heads, ntaps, in_size, offset=0, head_offset=0):
    nsamp = len(xs[0])
    buf, ptrs = upload(xs, offset)
    hbuf, hptrs = (None, None) if heads is None else upload(heads, head_offset)
    got, ms = ctx.stap_cov(ptrs, nsamp, in_size, ntaps, heads=hptrs)
    confirm_cov(ctx, kernel, len(xs), ntaps, nsamp, in_size)
    want = sr.cov_ref(xs, heads, ntaps)
    assert got.dtype == np.int64 and got.shape == want.shape and ms >= 0.0
    assert np.array_equal(got, want), (kernel, len(xs), ntaps, nsamp, in_size, np.argwhere(got != want)[:4].tolist())
    again, _ = ctx.stap_cov(ptrs, nsamp, in_size, ntaps, heads=hptrs)   # the same call twice gives the same numbers
    assert np.array_equal(again, got)
    del buf, hbuf
    return got


@pytest.mark.parametrize("nelem,ntaps", SHAPES)
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_at_every_edge(ctx, monkeypatch, kernel, in_size, nelem, ntaps):
    """nsamp 1, ntaps - 1 (0 with one tap: zeros, nothing launched), either side of a k-step, of one run and of three runs and a bit;
    heads for all, for none, for every other element, in turn"""
    set_kernel(monkeypatch, kernel)
    run = lim().gen_run if kernel == "generic" else lim().min_run * lim().k
    for i, nsamp in enumerate((1, ntaps - 1, 63, 64, 65, run - 1, run + 1, 3 * run + 7)):
        xs, heads = cut(in_size, nelem, ntaps, AT + i, nsamp, ("all", "none", "some")[i % 3])
        check_cov(ctx, kernel, xs, heads, ntaps, in_size)


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_sources_and_heads_that_are_not_16_byte_aligned(ctx, monkeypatch, kernel, in_size):
    set_kernel(monkeypatch, kernel)
    for k, offset in enumerate((4, 8, 12)):
        for nelem, ntaps, nsamp in ((3, 3, 64), (2, 4, 1000), (4, 5, 4097)):
            xs, heads = cut(in_size, nelem, ntaps, AT + offset, nsamp)
            check_cov(ctx, kernel, xs, heads, ntaps, in_size, offset=offset, head_offset=(8, 12, 4)[k])


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_the_extremes(ctx, monkeypatch, kernel, in_size):
    """all at the most negative value, heads too (the largest products there are), and mixed extremes"""
    set_kernel(monkeypatch, kernel)
    lo = -128 if in_size == 1 else -32768
    dtype = np.int8 if in_size == 1 else np.int16
    for nelem, ntaps in ((1, 1), (2, 4), (8, 4)):
        nsamp = 9001
        worst = [np.full((nsamp, 2), lo, dtype) for _ in range(nelem)]
        got = check_cov(ctx, kernel, worst, [np.full((ntaps - 1, 2), lo, dtype) for _ in range(nelem)], ntaps, in_size)
        assert (got[:, :, 0] == 2 * nsamp * lo * lo).all() and not got[:, :, 1].any()
        xs, heads = cut(in_size, nelem, ntaps, AT, nsamp, kind="extremes")
        check_cov(ctx, kernel, xs, heads, ntaps, in_size)


def test_the_planner_chooses_what_it_says(ctx, monkeypatch):
    set_kernel(monkeypatch, None)
    for in_size in (SC08, SC16):
        for nelem, ntaps in ((1, 1), (2, 4), (8, 4)):
            xs, heads = cut(in_size, nelem, ntaps, AT, 5000)
            check_cov(ctx, None, xs, heads, ntaps, in_size)
    assert ctx.stap_last_plan()[0] == "generic"                        # int16 has no matrix kernel


@pytest.mark.parametrize("nelem,ntaps", [(1, 1), (2, 5)], ids=["one tile", "off-diagonal tiles"])
def test_the_matrix_kernel_flushes_at_its_bound(ctx, monkeypatch, nelem, ntaps):
    """One full flush interval plus one k-step for every wave, every byte -128: the int32 entries of the rows in use stand at
    2^31 - 2^20 when they are flushed (tests/test_stap_plan.py multiplies that out on the CPU).  (1, 1) is the smallest shape the run
    geometry allows; (2, 5) has ten rows, so the tile below the diagonal flushes too -- both elements read the same 2^28 samples,
    512 MiB.  No head: row (e, t) is zero for its first t samples, so R[k][l] = 2^15 (nsamp - max(t_k, t_l)) and every imaginary
    part is 0; the closed form is checked against cov_ref on a piece."""
    import torch
    set_kernel(monkeypatch, "mfma")
    nsamp = lim().k * lim().max_grid * 4 * (lim().flush + 1)
    assert nsamp == 2 ** 28
    plan = sp.ask([("cov", nelem, ntaps, nsamp, 1, sp.FORCE_MFMA)])[0]
    assert plan.run == 4 * (lim().flush + 1) and plan.grid == lim().max_grid
    free, total = torch.cuda.mem_get_info()
    assert free >= 1 << 30, "the flush test needs 1 GiB of free device memory"
    buf = torch.full((2 * nsamp,), -128, dtype=torch.int8, device="cuda")
    got, _ = ctx.stap_cov([buf.data_ptr()] * nelem, nsamp, SC08, ntaps)
    assert ctx.stap_last_plan() == ("mfma", plan.grid, plan.run, nelem, ntaps)
    later = np.maximum.outer(np.arange(nelem * ntaps) % ntaps, np.arange(nelem * ntaps) % ntaps)

    def closed(n):
        want = np.zeros((nelem * ntaps, nelem * ntaps, 2), np.int64)
        want[:, :, 0] = 2 ** 15 * (n - later)
        return want

    assert np.array_equal(sr.cov_ref([np.full((4096, 2), -128, np.int8)] * nelem, None, ntaps), closed(4096))
    assert np.array_equal(got, closed(nsamp))
    del buf
    torch.cuda.empty_cache()


# ---- the combiner ------------------------------------------------------------------------------------------------------------------
def weights_at_the_bound(nelem, ntaps, signs):
    """sum |re| + |im| = 65535 exactly over the K weights, every re of sign signs[0] and every im of sign signs[1]; one weight: the
    largest int16 holds, 65534 where both are positive"""
    rows = nelem * ntaps
    if rows == 1:
        re = 32767 if signs[0] > 0 else -32768
        im = 32767 if signs[1] > 0 else -32768 if signs[0] > 0 else -32767
        w = np.array([[re, im]], np.int64)
    else:
        w = np.full((rows, 2), 65535 // (2 * rows), np.int64)
        w[0, 0] += 65535 - int(w.sum())
        w[:, 0] *= signs[0]
        w[:, 1] *= signs[1]
    assert int(np.abs(w).sum()) in ((65535,) if rows > 1 or signs != (1, 1) else (65534,)) and w.min() >= -32768 and w.max() <= 32767
    return w.astype(np.int16).reshape(nelem, ntaps, 2)


def run_combine(ctx, xs, heads, w, shift, out_size, dst_offset=0, offset=0, head_offset=0):
    import torch
    in_size = np.asarray(xs[0]).dtype.itemsize
    nsamp = len(xs[0])
    buf, ptrs = upload(xs, offset)
    hbuf, hptrs = (None, None) if heads is None else upload(heads, head_offset)
    olen = 2 * nsamp * out_size
    dst = torch.full((2 * PAD + olen + 16,), GUARD, dtype=torch.uint8, device="cuda")
    at = PAD + dst_offset
    clipped, ms = ctx.stap_combine(ptrs, nsamp, in_size, w, shift, out_size, dst.data_ptr() + at, heads=hptrs)
    got = dst.cpu().numpy()
    assert ms >= 0.0
    assert (got[:at] == GUARD).all() and (got[at + olen:] == GUARD).all(), "guard bytes of the destination changed"
    plan = sp.ask([("combine", nsamp, out_size, (dst.data_ptr() + at) % 16)])[0]
    name, grid, slot, elements, taps = ctx.stap_last_plan()
    assert (elements, taps) == (len(xs), np.asarray(w).shape[1])
    if plan is None:
        assert name is None
    else:
        assert (name, grid, slot) == ("combine", plan.grid, 16 // (2 * out_size))
    del buf, hbuf
    return got[at:at + olen].view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2).copy(), clipped


def check_combine(ctx, xs, heads, w, shift, out_size, **kw):
    want, wc = sr.combine_ref(xs, heads, w, shift, out_size)
    got, gc = run_combine(ctx, xs, heads, w, shift, out_size, **kw)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(xs), np.asarray(w).shape[1], len(xs[0]), shift, out_size, kw, "first differing sample", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


@pytest.mark.parametrize("nelem,ntaps", [(1, 1), (4, 2), (2, 5), (1, 8), (4, 8)])
@PAIRS
def test_combiner_at_every_edge(ctx, in_size, out_size, nelem, ntaps):
    """slot, wave and workgroup edges, spans shorter than the taps, heads for all, none and some, every alignment of dst and sources"""
    slot = 16 // (2 * out_size)
    sizes = [0, 1, ntaps - 1, slot - 1, slot, slot + 1, 64 * slot - 1, 64 * slot, 64 * slot + 1, 256 * slot - 1, 256 * slot, 256 * slot + 1, 3 * 256 * slot + 5]
    rng = np.random.default_rng(90 + 10 * in_size + out_size + nelem + ntaps)
    rows = nelem * ntaps
    for i, nsamp in enumerate(sizes):
        xs, heads = cut(in_size, nelem, ntaps, AT + 2 * i, nsamp, ("all", "none", "some")[i % 3])
        shift = (0, 14, 24)[i % 3]
        limw = min(65535 // (2 * rows), 32767) if shift else 3           # shift 0: small weights, so that not everything is clamped
        w = rng.integers(-limw, limw + 1, size=(nelem, ntaps, 2)).astype(np.int16)
        check_combine(ctx, xs, heads, w, shift, out_size, dst_offset=(0, 4, 8, 12)[i % 4], offset=(0, 4, 8, 12)[(i // 2) % 4], head_offset=(4, 0, 12, 8)[i % 4])


@pytest.mark.parametrize("signs", [(1, 1), (1, -1), (-1, 1), (-1, -1)], ids=["++", "+-", "-+", "--"])
@pytest.mark.parametrize("nelem,ntaps", [(1, 1), (1, 8), (8, 4)])
def test_combiner_with_weights_at_the_bound_against_the_extremes(ctx, nelem, ntaps, signs):
    """|acc| reaches 65535 * 32768 with int16 input: the sum must not wrap, whatever the signs"""
    w = weights_at_the_bound(nelem, ntaps, signs)
    clipped = 0
    for in_size in (SC08, SC16):
        lo = -128 if in_size == 1 else -32768
        dtype = np.int8 if in_size == 1 else np.int16
        worst = [np.full((777, 2), lo, dtype) for _ in range(nelem)]
        worst_heads = [np.full((ntaps - 1, 2), lo, dtype) for _ in range(nelem)]
        for out_size, shift in ((SC08, 24), (SC16, 14), (SC16, 0)):
            clipped += check_combine(ctx, worst, worst_heads, w, shift, out_size)
            xs, heads = cut(in_size, nelem, ntaps, AT, 777, kind="extremes")
            clipped += check_combine(ctx, xs, heads, w, shift, out_size, dst_offset=4)
    assert clipped > 0


# ---- the four identities, against the device's own earlier stages -----------------------------------------------------------------------
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_one_tap_is_the_devices_own_array_stage(ctx, monkeypatch, kernel, in_size):
    import torch
    set_kernel(monkeypatch, kernel)
    monkeypatch.delenv("GPSIQ_ARRAY_KERNEL", raising=False)
    for nelem in (1, 3, 8):
        xs, _ = cut(in_size, nelem, 1, AT, 6001, kind="extremes")
        buf, ptrs = upload(xs)
        a, _ = ctx.array_cov(ptrs, 6001, in_size)
        s, _ = ctx.stap_cov(ptrs, 6001, in_size, 1, heads=[ptrs[0]] * nelem)       # one tap: the heads are not read
        assert np.array_equal(s, a)
        w = np.random.default_rng(nelem).integers(-4000, 4001, size=(nelem, 2)).astype(np.int16)
        for out_size, shift in ((SC08, 20 if in_size == 2 else 13), (SC16, 12)):
            ya = torch.zeros(2 * 6001 * out_size, dtype=torch.uint8, device="cuda")
            ys = torch.zeros_like(ya)
            ca, _ = ctx.array_combine(ptrs, 6001, in_size, w, shift, out_size, ya.data_ptr())
            cs, _ = ctx.stap_combine(ptrs, 6001, in_size, w[:, None, :], shift, out_size, ys.data_ptr())
            assert torch.equal(ya, ys) and ca == cs
        del buf


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_the_rows_of_tap_zero_are_the_devices_own_array_covariance(ctx, monkeypatch, kernel, in_size):
    set_kernel(monkeypatch, kernel)
    for nelem, ntaps in ((2, 4), (3, 3), (8, 4), (4, 8)):
        xs, heads = cut(in_size, nelem, ntaps, AT, 5003)
        buf, ptrs = upload(xs)
        a, _ = ctx.array_cov(ptrs, 5003, in_size)
        idx = np.arange(nelem) * ntaps
        for hs in (None, heads, cut(in_size, nelem, ntaps, AT + 100, 1, kind="extremes")[1]):
            hbuf, hptrs = (None, None) if hs is None else upload(hs)
            s, _ = ctx.stap_cov(ptrs, 5003, in_size, ntaps, heads=hptrs)
            assert np.array_equal(s[np.ix_(idx, idx)], a)
            del hbuf
        del buf


@PAIRS
def test_one_element_is_the_devices_own_complex_filter(ctx, in_size, out_size):
    import torch
    rng = np.random.default_rng(17)
    for ntaps, shift in ((1, 14), (2, 15), (5, 16), (8, 24), (8, 0)):
        xs, heads = cut(in_size, 1, ntaps, AT, 3001, kind="extremes")
        lim_w = min(65535 // (2 * ntaps), 32767) if shift else 2
        taps = rng.integers(-lim_w, lim_w + 1, size=(ntaps, 2)).astype(np.int16)
        for hs in (heads, None):
            got, gc = run_combine(ctx, xs, hs, taps[None], shift, out_size)
            src, (sp_,) = upload(xs)
            hbuf, hp = (None, [0]) if hs is None or ntaps == 1 else upload(hs)
            dst = torch.zeros(2 * 3001 * out_size, dtype=torch.uint8, device="cuda")
            nout, fc, _ = ctx.cfilter(3001, in_size, sp_, taps, shift, 1, 0, out_size, dst.data_ptr(), head_ptr=hp[0] or None)
            filt = dst.cpu().numpy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2)
            assert nout == 3001 and np.array_equal(got, filt) and gc == fc, (ntaps, shift, hs is None)
            del src, hbuf


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_the_combined_stream_is_the_quadratic_form(ctx, monkeypatch, kernel, in_size):
    """shift 0, nothing clamped: array_cov of the device's combined stream equals w R w^H from stap_cov of the inputs, exactly"""
    import torch
    set_kernel(monkeypatch, kernel)
    for nelem, ntaps in ((2, 4), (4, 5)):
        nsamp, rows = 12345, nelem * ntaps
        xs, heads = cut(in_size, nelem, ntaps, AT, nsamp)
        if in_size == 2:
            xs, heads = [(x // 256).astype(np.int16) for x in xs], [(h // 256).astype(np.int16) for h in heads]     # |x| <= 128, as int8
        limw = 32767 // (rows * 2 * 128)                                # |y| <= K * 2 * limw * 128, inside int16
        w = np.random.default_rng(77).integers(-limw, limw + 1, size=(nelem, ntaps, 2)).astype(np.int16)
        buf, ptrs = upload(xs)
        hbuf, hptrs = upload(heads)
        r, _ = ctx.stap_cov(ptrs, nsamp, in_size, ntaps, heads=hptrs)
        y = torch.zeros(4 * nsamp, dtype=torch.uint8, device="cuda")
        clipped, _ = ctx.stap_combine(ptrs, nsamp, in_size, w, 0, SC16, y.data_ptr(), heads=hptrs)
        assert clipped == 0
        ry, _ = ctx.array_cov([y.data_ptr()], nsamp, SC16)
        assert sr.quadratic_form(w, r) == (int(ry[0, 0, 0]), 0) and ry[0, 0, 1] == 0
        del buf, hbuf


# ---- continuation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_a_span_in_pieces_adds_up_to_one_call(ctx, monkeypatch, kernel, in_size):
    """pieces shorter than ntaps - 1 among them; every piece's head is the last ntaps - 1 samples before it"""
    set_kernel(monkeypatch, kernel)
    nelem, ntaps, nsamp = 3, 6, 9000
    out_size, shift = SC08, 9 if in_size == 1 else 17
    w = np.random.default_rng(3).integers(-900, 901, size=(nelem, ntaps, 2)).astype(np.int16)
    xs, heads = cut(in_size, nelem, ntaps, AT, nsamp)
    whole = check_cov(ctx, kernel, xs, heads, ntaps, in_size)
    want_y, want_c = sr.combine_ref(xs, heads, w, shift, out_size)
    assert want_c > 0
    cuts = [0, 2, 3, 7, 8, 64, 4100, 4101, 4104, nsamp]
    total, ys, count = np.zeros_like(whole), [], 0
    for lo, hi in zip(cuts, cuts[1:]):
        pxs, ph = cut(in_size, nelem, ntaps, AT + lo, hi - lo)
        buf, ptrs = upload(pxs, offset=(0, 4, 8, 12)[lo % 4])
        hbuf, hptrs = upload(ph)
        piece, _ = ctx.stap_cov(ptrs, hi - lo, in_size, ntaps, heads=hptrs)
        total += piece
        y, c = run_combine(ctx, pxs, ph, w, shift, out_size, dst_offset=(0, 4, 8, 12)[hi % 4])
        ys.append(y)
        count += c
        del buf, hbuf
    assert np.array_equal(total, whole) and np.array_equal(np.concatenate(ys), want_y) and count == want_c


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    import torch
    x = [torch.zeros(4096, dtype=torch.uint8, device="cuda") for _ in range(9)]
    ptrs = [t.data_ptr() for t in x]
    hd = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    w22 = np.zeros((2, 2, 2), np.int16)
    w22[0, 0, 0] = 1

    def code(call):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call()
        return e.value.code

    def wk(nelem, ntaps):
        return np.zeros((nelem, ntaps, 2), np.int16)

    e_arg = code(lambda: ctx.stap_cov(ptrs[:2], -1, SC08, 2))
    over = np.array([[[32767, 0], [0, 0]], [[32767, 2], [0, 0]]], np.int16)
    e_range = code(lambda: ctx.stap_combine(ptrs[:2], 100, SC08, over, 0, SC08, dst.data_ptr()))
    assert e_arg != e_range
    over[1, 0, 1], over[1, 1, 1] = 0, 1                                  # the bound itself, 65535, spread over two taps
    assert ctx.stap_combine(ptrs[:2], 100, SC08, over, 0, SC08, dst.data_ptr())[0] == 0
    bad = [lambda: ctx.stap_cov([], 10, SC08, 2), lambda: ctx.stap_cov(ptrs, 10, SC08, 2),                    # no element, nine elements
           lambda: ctx.stap_cov(ptrs[:2], 10, SC08, 0), lambda: ctx.stap_cov(ptrs[:2], 10, SC08, 9),              # no tap, nine taps
           lambda: ctx.stap_cov(ptrs[:5], 10, SC08, 7), lambda: ctx.stap_cov(ptrs[:8], 10, SC08, 5),              # 35 and 40 rows
           lambda: ctx.stap_cov(ptrs[:2], 10, 3, 2), lambda: ctx.stap_cov(ptrs[:2], 10, 0, 2),                    # bad formats
           lambda: ctx.stap_cov([ptrs[0], 0], 10, SC08, 2), lambda: ctx.stap_cov([ptrs[0] + 2, ptrs[1]], 10, SC08, 2),   # null, misaligned source
           lambda: ctx.stap_cov(ptrs[:2], 10, SC08, 2, heads=[hd.data_ptr() + 2, 0]),                            # misaligned head
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, 0, SC08, dst.data_ptr(), heads=[0, hd.data_ptr() + 2]),
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, 0, 3, dst.data_ptr()), lambda: ctx.stap_combine(ptrs[:2], 10, 4, w22, 0, SC08, dst.data_ptr()),
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, -1, SC08, dst.data_ptr()), lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, 25, SC08, dst.data_ptr()),
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, 0, SC08, 0), lambda: ctx.stap_combine([ptrs[0], 0], 10, SC08, w22, 0, SC08, dst.data_ptr()),
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, w22, 0, SC08, dst.data_ptr() + 2), lambda: ctx.stap_combine(ptrs[:2], -1, SC08, w22, 0, SC08, dst.data_ptr()),
           lambda: ctx.stap_combine(ptrs[:2], 10, SC08, wk(2, 9), 0, SC08, dst.data_ptr()), lambda: ctx.stap_combine(ptrs[:5], 10, SC08, wk(5, 7), 0, SC08, dst.data_ptr()),
           # dst over the second source: its first byte, its last byte, and a wider output reaching into it from below
           lambda: ctx.stap_combine(ptrs[:2], 100, SC08, w22, 0, SC08, ptrs[1]), lambda: ctx.stap_combine(ptrs[:2], 100, SC08, w22, 0, SC08, ptrs[1] + 196),
           lambda: ctx.stap_combine([ptrs[0], ptrs[0] + 400], 100, SC08, w22, 0, SC16, ptrs[0] + 4),
           # dst over a head: a head of one sample (two taps) is two bytes, at the start of dst and at its last byte
           lambda: ctx.stap_combine(ptrs[:2], 100, SC08, w22, 0, SC08, dst.data_ptr(), heads=[0, dst.data_ptr()]),
           lambda: ctx.stap_combine(ptrs[:2], 100, SC08, w22, 0, SC08, dst.data_ptr(), heads=[dst.data_ptr() + 196, 0])]
    for k, call in enumerate(bad):
        assert code(call) == e_arg, k
    # a null pointer is no fault where there is nothing to read or write
    cov, _ = ctx.stap_cov([0, 0], 0, SC16, 4)
    assert cov.shape == (8, 8, 2) and not cov.any() and ctx.stap_combine([0, 0], 0, SC08, w22, 0, SC08, 0)[0] == 0
    # side by side is no overlap: the head ends where dst begins
    assert ctx.stap_combine([ptrs[0], ptrs[0] + 200], 100, SC08, w22, 0, SC08, ptrs[0] + 400)[0] == 0
    assert ctx.stap_combine(ptrs[:2], 100, SC08, w22, 0, SC08, dst.data_ptr() + 4, heads=[dst.data_ptr(), dst.data_ptr() + 204])[0] == 0
