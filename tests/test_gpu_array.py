"""gpsiq_array_cov and gpsiq_array_combine on the MI355X: every int64 word of the covariance, every output byte, every guard byte and
every count equals tests/_array_ref.py's restatement of the contract (include/gpsiq_rows.h, "Array"), on every kernel that can serve
-- array_cov_generic (both formats), array_cov_mfma (int8) -- each forced through GPSIQ_ARRAY_KERNEL and confirmed with
gpsiq_array_last_plan, whose plan is held to the planner's (tests/array_plan.cpp).  The shapes are the smallest at which a kernel can
go wrong: both sides of a k-step, of a chunk, of a workgroup's run and of two runs, of a lane's slot, a wave and a workgroup; sources
at addresses that are 4-byte but not 16-byte aligned; the extremes of both formats; and the one span at which every wave of the matrix
kernel takes a full flush interval plus one k-step.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import _array_plan as ap
import _array_ref as ar
import _cfilter_ref as cr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
PAD = 64
NELEMS = [1, 2, 3, 7, 8]
SERVING = [("generic", SC08), ("generic", SC16), ("mfma", SC08)]
SERVING_IDS = ["generic-int8", "generic-int16", "mfma-int8"]
SHIFTS = [0, 14, 24]
FORCE = {"generic": ap.FORCE_GENERIC, "mfma": ap.FORCE_MFMA, None: ap.AUTO}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def lim():
    return ap.limits()


@functools.lru_cache(maxsize=None)
def pool(size, kind="random"):
    """eight streams of a format every case cuts its elements from (computed once, never written)"""
    p = ar.streams(np.random.default_rng(4100 + size + len(kind)), 8, 20000, size, kind)
    for x in p:
        x.setflags(write=False)
    return tuple(p)


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_ARRAY_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_ARRAY_KERNEL", kernel)


def upload(xs, offset=0):
    """the streams in ONE device buffer, each at a 16-byte aligned address plus `offset` bytes (a multiple of 4) -> (buffer, pointers)"""
    import torch
    assert offset % 4 == 0
    sizes = [np.asarray(x).nbytes for x in xs]
    stride = [(-(-(s + offset) // 16) + 1) * 16 for s in sizes]
    raw = np.zeros(sum(stride) + 16, np.uint8)
    at, ptrs = 0, []
    for x, s, st in zip(xs, sizes, stride):
        raw[at + offset:at + offset + s] = np.ascontiguousarray(x).view(np.uint8).ravel()
        ptrs.append(at + offset)
        at += st
    buf = torch.from_numpy(raw).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, [buf.data_ptr() + p for p in ptrs]


def confirm_cov(ctx, kernel, nelem, nsamp, in_size):
    plan = ap.ask([("cov", nelem, nsamp, in_size, FORCE[kernel])])[0]
    name, grid, run, elements = ctx.array_last_plan()
    if plan is None:
        assert name is None and elements == nelem
        return
    assert (name, grid, run, elements) == (ap.KERNELS[plan.kernel], plan.grid, plan.run, nelem)
    if kernel is not None:
        assert name == kernel


def check_cov(ctx, kernel, xs, in_size, offset=0):
    nsamp = len(xs[0])
    buf, ptrs = upload(xs, offset)
    got, ms = ctx.array_cov(ptrs, nsamp, in_size)
    confirm_cov(ctx, kernel, len(xs), nsamp, in_size)
    want = ar.cov_ref(xs) if nsamp else np.zeros((len(xs), len(xs), 2), np.int64)
    assert got.dtype == np.int64 and got.shape == want.shape and ms >= 0.0
    assert np.array_equal(got, want), (kernel, len(xs), nsamp, in_size, np.argwhere(got != want)[:4].tolist())
    again, _ = ctx.array_cov(ptrs, nsamp, in_size)                      # the same call twice gives the same numbers
    assert np.array_equal(again, got)
    del buf
    return got


@pytest.mark.parametrize("nelem", NELEMS)
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_at_the_small_edges(ctx, monkeypatch, kernel, in_size, nelem):
    set_kernel(monkeypatch, kernel)
    for i, nsamp in enumerate((0, 1, 63, 64, 65, 255, 256, 257)):
        xs = [x[3 * i:3 * i + nsamp] for x in pool(in_size)[:nelem]]
        check_cov(ctx, kernel, xs, in_size)


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_either_side_of_one_run_and_of_two(ctx, monkeypatch, kernel, in_size):
    set_kernel(monkeypatch, kernel)
    run = lim().gen_run if kernel == "generic" else lim().min_run * lim().k
    for i, nsamp in enumerate((run - 1, run, run + 1, 2 * run - 1, 2 * run, 2 * run + 1)):
        nelem = NELEMS[i % len(NELEMS)]
        xs = [x[i:i + nsamp] for x in pool(in_size)[:nelem]]
        check_cov(ctx, kernel, xs, in_size)
    # more runs than one pass of the grid would take if it were small, and every element count at a ragged length
    for nelem in NELEMS:
        check_cov(ctx, kernel, [x[:19999 - nelem] for x in pool(in_size)[:nelem]], in_size)


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_sources_that_are_not_16_byte_aligned(ctx, monkeypatch, kernel, in_size):
    set_kernel(monkeypatch, kernel)
    for offset in (4, 8, 12):
        for nsamp in (64, 1000, 4097):
            check_cov(ctx, kernel, [x[offset:offset + nsamp] for x in pool(in_size)[:3]], in_size, offset=offset)


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_the_extremes(ctx, monkeypatch, kernel, in_size):
    """all at the most negative value (the largest products there are), and mixed extremes"""
    set_kernel(monkeypatch, kernel)
    lo = -128 if in_size == 1 else -32768
    dtype = np.int8 if in_size == 1 else np.int16
    for nelem in (1, 8):
        nsamp = 9001
        got = check_cov(ctx, kernel, [np.full((nsamp, 2), lo, dtype) for _ in range(nelem)], in_size)
        assert got[0, 0].tolist() == [2 * nsamp * lo * lo, 0]
        check_cov(ctx, kernel, [x[:nsamp] for x in pool(in_size, "extremes")[:nelem]], in_size)


def test_the_planner_chooses_what_it_says(ctx, monkeypatch):
    set_kernel(monkeypatch, None)
    for in_size in (SC08, SC16):
        for nelem in (1, 2, 8):
            check_cov(ctx, None, [x[:5000] for x in pool(in_size)[:nelem]], in_size)
    name, _, _, _ = ctx.array_last_plan()
    assert name == "generic"                                           # int16 has no matrix kernel


@pytest.mark.parametrize("nelem", [1, 8])
def test_the_matrix_kernel_flushes_at_its_bound(ctx, monkeypatch, nelem):
    """One full flush interval plus one k-step for every wave, every byte of every element -128: the int32 entries of the rows in use
    (two with one element, all 256 entries of the tile with eight) stand at 2^31 - 2^20 when they are flushed
    (tests/test_array_plan.py multiplies that out on the CPU).  2^29 samples an element, 1 GiB each; the restatement of constant
    streams is its closed form, 2 nsamp 2^14 in every real part and 0 in every imaginary part, checked against cov_ref on a piece."""
    import torch
    set_kernel(monkeypatch, "mfma")
    nsamp = lim().k * lim().max_grid * 4 * (lim().flush + 1)
    assert nsamp == 2 ** 29
    plan = ap.ask([("cov", nelem, nsamp, 1, ap.FORCE_MFMA)])[0]
    assert plan.run == 4 * (lim().flush + 1) and plan.grid == lim().max_grid
    free, total = torch.cuda.mem_get_info()
    assert free >= (nelem + 1) << 30, "the flush test needs %d GiB of free device memory" % (nelem + 1)
    buf = torch.full((nelem, 2 * nsamp), -128, dtype=torch.int8, device="cuda")
    got, _ = ctx.array_cov([buf[e].data_ptr() for e in range(nelem)], nsamp, SC08)
    assert ctx.array_last_plan() == ("mfma", plan.grid, plan.run, nelem)
    piece = ar.cov_ref([np.full((4096, 2), -128, np.int8) for _ in range(nelem)])
    want = np.zeros((nelem, nelem, 2), np.int64)
    want[:, :, 0] = 2 * 4096 * 2 ** 14
    assert np.array_equal(piece, want)
    want[:, :, 0] = 2 * nsamp * 2 ** 14
    assert np.array_equal(got, want)
    del buf
    torch.cuda.empty_cache()


# ---- the combiner ------------------------------------------------------------------------------------------------------------------
def weights_at_the_bound(nelem, signs):
    """sum |re| + |im| = 65535 exactly, every re of sign signs[0] and every im of sign signs[1]; one element: the largest int16 holds,
    65534 where both are positive"""
    if nelem == 1:
        re = 32767 if signs[0] > 0 else -32768
        im = 32767 if signs[1] > 0 else -32768 if signs[0] > 0 else -32767
        w = np.array([[re, im]], np.int64)
    else:
        w = np.full((nelem, 2), 65535 // (2 * nelem), np.int64)
        w[0, 0] += 65535 - int(w.sum())
        w[:, 0] *= signs[0]
        w[:, 1] *= signs[1]
    assert int(np.abs(w).sum()) in ((65535,) if nelem > 1 or signs != (1, 1) else (65534,)) and w.min() >= -32768 and w.max() <= 32767
    return w.astype(np.int16)


def run_combine(ctx, xs, w, shift, out_size, dst_offset=0, offset=0):
    import torch
    in_size = np.asarray(xs[0]).dtype.itemsize
    nsamp = len(xs[0])
    buf, ptrs = upload(xs, offset)
    olen = 2 * nsamp * out_size
    dst = torch.full((2 * PAD + olen + 16,), GUARD, dtype=torch.uint8, device="cuda")
    at = PAD + dst_offset
    clipped, ms = ctx.array_combine(ptrs, nsamp, in_size, w, shift, out_size, dst.data_ptr() + at)
    got = dst.cpu().numpy()
    assert ms >= 0.0
    assert (got[:at] == GUARD).all() and (got[at + olen:] == GUARD).all(), "guard bytes of the destination changed"
    plan = ap.ask([("combine", nsamp, out_size, (dst.data_ptr() + at) % 16)])[0]
    name, grid, slot, elements = ctx.array_last_plan()
    if plan is None:
        assert name is None
    else:
        assert (name, grid, slot, elements) == ("combine", plan.grid, 16 // (2 * out_size), len(xs))
    del buf
    return got[at:at + olen].view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2).copy(), clipped


def check_combine(ctx, xs, w, shift, out_size, **kw):
    want, wc = ar.combine_ref(xs, w, shift, out_size)
    got, gc = run_combine(ctx, xs, w, shift, out_size, **kw)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(xs), len(xs[0]), shift, out_size, kw, "first differing sample", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


@pytest.mark.parametrize("nelem", [1, 8])
@pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)], ids=["8to8", "8to16", "16to8", "16to16"])
def test_combiner_at_every_edge(ctx, in_size, out_size, nelem):
    slot = 16 // (2 * out_size)
    sizes = [0, 1, slot - 1, slot, slot + 1, 64 * slot - 1, 64 * slot, 64 * slot + 1, 256 * slot - 1, 256 * slot, 256 * slot + 1, 3 * 256 * slot + 5]
    rng = np.random.default_rng(90 + 10 * in_size + out_size + nelem)
    for i, nsamp in enumerate(sizes):
        xs = [x[2 * i:2 * i + nsamp] for x in pool(in_size)[:nelem]]
        shift = SHIFTS[i % 3]
        limw = min(65535 // (2 * nelem), 32767) if shift else 3          # shift 0: small weights, so that not everything is clamped
        w = rng.integers(-limw, limw + 1, size=(nelem, 2)).astype(np.int16)
        check_combine(ctx, xs, w, shift, out_size, dst_offset=(0, 4, 8, 12)[i % 4], offset=(0, 4, 8, 12)[(i // 2) % 4])


@pytest.mark.parametrize("signs", [(1, 1), (1, -1), (-1, 1), (-1, -1)], ids=["++", "+-", "-+", "--"])
@pytest.mark.parametrize("nelem", [1, 8])
def test_combiner_with_weights_at_the_bound_against_the_extremes(ctx, nelem, signs):
    """|acc| reaches 65535 * 32768 with int16 input: the sum must not wrap, whatever the signs"""
    w = weights_at_the_bound(nelem, signs)
    clipped = 0
    for in_size in (SC08, SC16):
        lo = -128 if in_size == 1 else -32768
        dtype = np.int8 if in_size == 1 else np.int16
        worst = [np.full((777, 2), lo, dtype) for _ in range(nelem)]
        for out_size, shift in ((SC08, 24), (SC16, 14), (SC16, 0)):
            clipped += check_combine(ctx, worst, w, shift, out_size)
            clipped += check_combine(ctx, [x[:777] for x in pool(in_size, "extremes")[:nelem]], w, shift, out_size, dst_offset=4)
    assert clipped > 0


def test_refusals(ctx):
    import torch
    x = [torch.zeros(4096, dtype=torch.uint8, device="cuda") for _ in range(9)]
    ptrs = [t.data_ptr() for t in x]
    dst = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    w2 = np.array([[1, 0], [0, 1]], np.int16)

    def code(call):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call()
        return e.value.code

    e_arg = code(lambda: ctx.array_cov(ptrs[:2], -1, SC08))
    e_range = code(lambda: ctx.array_combine(ptrs[:2], 100, SC08, [[32767, 0], [32767, 2]], 0, SC08, dst.data_ptr()))
    assert e_arg != e_range
    assert ctx.array_combine(ptrs[:2], 100, SC08, [[32767, 0], [32767, 1]], 0, SC08, dst.data_ptr())[0] == 0      # the bound itself: 65535
    bad = [lambda: ctx.array_cov([], 10, SC08), lambda: ctx.array_cov(ptrs, 10, SC08),                  # no element, nine elements
           lambda: ctx.array_cov(ptrs[:2], 10, 3), lambda: ctx.array_cov(ptrs[:2], 10, 0),                # bad formats
           lambda: ctx.array_cov([ptrs[0], 0], 10, SC08), lambda: ctx.array_cov([ptrs[0] + 2, ptrs[1]], 10, SC08),   # null, misaligned
           lambda: ctx.array_combine(ptrs[:2], 10, SC08, w2, 0, 3, dst.data_ptr()), lambda: ctx.array_combine(ptrs[:2], 10, 4, w2, 0, SC08, dst.data_ptr()),
           lambda: ctx.array_combine(ptrs[:2], 10, SC08, w2, -1, SC08, dst.data_ptr()), lambda: ctx.array_combine(ptrs[:2], 10, SC08, w2, 25, SC08, dst.data_ptr()),
           lambda: ctx.array_combine(ptrs[:2], 10, SC08, w2, 0, SC08, 0), lambda: ctx.array_combine([ptrs[0], 0], 10, SC08, w2, 0, SC08, dst.data_ptr()),
           lambda: ctx.array_combine(ptrs[:2], 10, SC08, w2, 0, SC08, dst.data_ptr() + 2), lambda: ctx.array_combine(ptrs[:2], -1, SC08, w2, 0, SC08, dst.data_ptr()),
           # dst over the second source: its first byte, its last byte, and a wider output reaching into it from below
           lambda: ctx.array_combine(ptrs[:2], 100, SC08, w2, 0, SC08, ptrs[1]), lambda: ctx.array_combine(ptrs[:2], 100, SC08, w2, 0, SC08, ptrs[1] + 196),
           lambda: ctx.array_combine([ptrs[0], ptrs[0] + 400], 100, SC08, w2, 0, SC16, ptrs[0] + 4)]
    for k, call in enumerate(bad):
        assert code(call) == e_arg, k
    # a null pointer is no fault where there is nothing to read or write
    cov, _ = ctx.array_cov([0, 0], 0, SC16)
    assert not cov.any() and ctx.array_combine([0, 0], 0, SC08, w2, 0, SC08, 0)[0] == 0
    # side by side is no overlap
    assert ctx.array_combine([ptrs[0], ptrs[0] + 200], 100, SC08, w2, 0, SC08, ptrs[0] + 400)[0] == 0


# ---- the two device identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_size,out_size", [(1, 1), (1, 2), (2, 1), (2, 2)], ids=["8to8", "8to16", "16to8", "16to16"])
def test_one_element_is_the_devices_own_complex_filter_with_one_tap(ctx, in_size, out_size):
    import torch
    x = pool(in_size, "extremes")[0][:3001]
    for w, shift in (([[32767, -32768]], 14), ([[-3, 2]], 0), ([[0, 1]], 0)):
        got, gc = run_combine(ctx, [x], np.array(w, np.int16), shift, out_size)
        src = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda()
        dst = torch.zeros(2 * len(x) * out_size, dtype=torch.uint8, device="cuda")
        nout, fc, _ = ctx.cfilter(len(x), in_size, src.data_ptr(), np.array(w, np.int16), shift, 1, 0, out_size, dst.data_ptr())
        filt = dst.cpu().numpy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2)
        assert nout == len(x) and np.array_equal(got, filt) and gc == fc
        want, wc = cr.cfilter_ref(x, None, w, shift, 1, 0, out_size)
        assert np.array_equal(got, want) and gc == wc


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=SERVING_IDS)
def test_covariance_of_the_combined_stream_is_the_quadratic_form(ctx, monkeypatch, kernel, in_size):
    """shift 0, nothing clamped: array_cov of the device's combined stream equals w R w^H from array_cov of the inputs, exactly"""
    import torch
    set_kernel(monkeypatch, kernel)
    nelem, nsamp = 4, 12345
    xs = [x[:nsamp] for x in pool(in_size)[:nelem]]
    limw = 30
    if in_size == 2:
        xs = [(x // 64).astype(np.int16) for x in xs]                  # |y| <= 4 * 2 * 7 * 512, inside int16
        limw = 7
    w = np.random.default_rng(77).integers(-limw, limw + 1, size=(nelem, 2)).astype(np.int16)
    buf, ptrs = upload(xs)
    r, _ = ctx.array_cov(ptrs, nsamp, in_size)
    y = torch.zeros(4 * nsamp, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.array_combine(ptrs, nsamp, in_size, w, 0, SC16, y.data_ptr())
    assert clipped == 0
    ry, _ = ctx.array_cov([y.data_ptr()], nsamp, SC16)                 # (int16: the generic kernel, whatever is forced)
    assert ar.quadratic_form(w, r) == (int(ry[0, 0, 0]), 0) and ry[0, 0, 1] == 0
    del buf
