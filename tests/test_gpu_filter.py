"""gpsiq_filter on the MI355X: every output byte, every guard byte and every count equals tests/_filter_ref.py's restatement of the
contract (include/gpsiq_rows.h, "Filter"), on both kernels (GPSIQ_FILTER_KERNEL) and on the default path, whose choice is held to the
planner's (tests/filter_plan.cpp).  The spans are random full-range elements -- the kernels are pure functions of the stream --
and every destination lies between guard bytes of 0x7f that must not change.  The shapes are the smallest at which a kernel can
go wrong: both sides of a wave's tile, of a workgroup's run of outputs and of the history, and spans that end before the first
output.  Run with -m gpu."""
import numpy as np
import pytest

import _filter_plan as fp
import _filter_ref as fr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
PAD = 64                         # guard bytes either side of a destination
NTAPS = [1, 2, 16, 17, 63, 64, 65, 512]
DECIMS = [1, 2, 3, 4, 16]
SHIFTS = [0, 14, 24]
FORCE = {"generic": fp.GENERIC, "mfma": fp.MFMA, None: fp.AUTO}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """full-range samples of either format every case cuts its span and head from (computed once, never written)"""
    rng = np.random.default_rng(77)
    p = {ss: fr.full_range(rng, 40000, ss) for ss in (SC08, SC16)}
    for a in p.values():
        a.setflags(write=False)
    return p


def taps_for(ntaps, kind="mixed", seed=0):
    """mixed: both signs, sum |taps| well inside the range; full: sum |taps| = 65535 exactly, every tap inside two signed bytes"""
    rng = np.random.default_rng(1000 * ntaps + seed)
    if kind == "mixed":
        return rng.integers(-(60000 // ntaps // 2) - 1, 60000 // ntaps // 2 + 2, size=ntaps).astype(np.int16) if ntaps > 1 else np.array([-3], np.int16)
    t = rng.integers(-20, 21, size=ntaps).astype(np.int64)
    for k in range(ntaps):
        add = min(65535 - int(np.abs(t).sum()), 32639 - abs(int(t[k])))
        t[k] += add * (1 if t[k] >= 0 else -1)
    assert int(np.abs(t).sum()) == 65535
    return t.astype(np.int16)


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_FILTER_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_FILTER_KERNEL", kernel)


def run_filter(ctx, x, head, taps, shift, decim, phase, out_size, skew=0):
    """x [n, 2], head [ntaps - 1, 2] or None -> (out [nout, 2] as the device wrote it, clipped); guards compared.  skew: bytes the span
    starts past an 8-byte boundary"""
    import torch
    in_size = x.dtype.itemsize
    nsamp = len(x)
    nout = fr.span(nsamp, decim, phase)[0]
    raw = np.zeros(skew + 8 + x.nbytes, np.uint8)
    raw[skew:skew + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).ravel()
    src = torch.from_numpy(raw).cuda()
    hd = None if head is None else torch.from_numpy(np.ascontiguousarray(head).view(np.uint8).ravel().copy()).cuda()
    olen = 2 * nout * out_size
    dst = torch.full((2 * PAD + olen,), GUARD, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 8 == 0 and dst.data_ptr() % 4 == 0
    got_n, clipped, ms = ctx.filter(nsamp, in_size, src.data_ptr() + skew, taps, shift, decim, phase, out_size, dst.data_ptr() + PAD,
                                    head_ptr=None if hd is None or not len(hd) else hd.data_ptr())
    got = dst.cpu().numpy()
    assert got_n == nout and ms >= 0.0
    assert (got[:PAD] == GUARD).all() and (got[PAD + olen:] == GUARD).all(), "guard bytes of the destination changed"
    return got[PAD:PAD + olen].view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2).copy(), clipped


def check(ctx, x, head, taps, shift, decim, phase, out_size, skew=0):
    want, wc = fr.filter_ref(x, head, taps, shift, decim, phase, out_size)
    got, gc = run_filter(ctx, x, head, taps, shift, decim, phase, out_size, skew)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(x), len(taps), shift, decim, phase, "first differing output", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


def span_lengths(ntaps, decim, phase, run):
    """nsamp: one sample, both sides of the history, one workgroup's run of outputs -1 / +0 / +1 in input samples, two runs + 3, and
    spans that end at and just behind the first output"""
    full = phase + (run - 1) * decim + 1                             # the shortest span with `run` outputs
    return sorted({1, max(ntaps - 1, 1), ntaps, full - 1, full, full + 1, phase + (2 * run - 1) * decim + 1 + 3, max(phase, 1), phase + 1})


@pytest.mark.parametrize("kernel", ["generic", "mfma", None], ids=["generic", "mfma", "default"])
@pytest.mark.parametrize("ntaps", NTAPS)
def test_int8_sweep_of_taps_decimations_phases_and_lengths(ctx, pool, monkeypatch, kernel, ntaps):
    set_kernel(monkeypatch, kernel)
    taps = taps_for(ntaps)
    cases = []
    for decim in DECIMS:
        for phase in sorted({0, decim - 1}):
            run = fp.plan(10 ** 6, SC08, ntaps, decim, phase, int(taps.max()), FORCE[kernel]).run
            for nsamp in span_lengths(ntaps, decim, phase, run):
                cases.append((decim, phase, nsamp))
    plans = fp.ask([("plan", n, SC08, ntaps, d, ph, int(taps.max()), FORCE[kernel]) for d, ph, n in cases])
    for i, ((decim, phase, nsamp), plan) in enumerate(zip(cases, plans)):
        x = pool[SC08][i:i + nsamp]
        head = None if i % 2 else pool[SC08][30000 + i:30000 + i + ntaps - 1]
        check(ctx, x, head, taps, SHIFTS[i % 3], decim, phase, SC08)
        name, grid, run, pieces = ctx.filter_last_plan()
        if isinstance(plan, fp.Nothing):                             # the span ends before its first output
            assert name is None and nsamp <= phase
            continue
        assert (name, grid, run, pieces) == (fp.KERNELS[plan.kernel], plan.grid, plan.run, 0), (decim, phase, nsamp)
        if kernel is not None:
            assert name == kernel


def test_a_span_that_ends_before_the_first_output_writes_nothing(ctx, pool, monkeypatch):
    set_kernel(monkeypatch, None)
    taps = taps_for(17)
    for decim, phase, nsamp in [(4, 3, 3), (4, 3, 2), (16, 15, 15), (16, 15, 1), (3, 2, 0), (1, 0, 0)]:
        got, clipped = run_filter(ctx, pool[SC16][:nsamp], None, taps, 14, decim, phase, SC16)
        assert len(got) == 0 and clipped == 0 and ctx.filter_last_plan()[0] is None


@pytest.mark.parametrize("kernel,in_size,out_size", [("generic", SC08, SC08), ("generic", SC08, SC16), ("generic", SC16, SC08), ("generic", SC16, SC16),
                                                     ("mfma", SC08, SC08), ("mfma", SC08, SC16)])
def test_format_pairs_shifts_and_a_clamp_that_fires(ctx, pool, monkeypatch, kernel, in_size, out_size):
    """taps of both signs with sum |taps| = 65535 against a full-scale stream: at shift 0 nearly every element is clamped, at 14 some are,
    and the count is the reference's"""
    set_kernel(monkeypatch, kernel)
    counts = []
    for ntaps, decim, phase, nsamp in [(17, 1, 0, 1500), (65, 4, 3, 4131), (512, 3, 1, 3000)]:
        taps = taps_for(ntaps, "full")
        for shift in SHIFTS:
            counts.append(check(ctx, pool[in_size][5:5 + nsamp], pool[in_size][20000:20000 + ntaps - 1], taps, shift, decim, phase, out_size))
        assert ctx.filter_last_plan()[0] == kernel
    assert counts[0] > 0 and sum(counts) > counts[0]
    # the extremes alone: every element the most negative value, every tap negative
    x = np.full((300, 2), -128 if in_size == SC08 else -32768, dtype=pool[in_size].dtype)
    taps = np.full(15, -4369, np.int16)                              # 15 * 4369 = 65535
    for shift in (0, 8, 16):
        check(ctx, x, x[:14], taps, shift, 2, 1, out_size)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_source_aligned_to_4_bytes_and_no_more_and_the_same_call_twice(ctx, pool, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    taps = taps_for(33)
    x, head = pool[SC08][100:100 + 2777], pool[SC08][9000:9032]
    check(ctx, x, head, taps, 9, 3, 2, SC16, skew=4)
    a = run_filter(ctx, x, head, taps, 9, 3, 2, SC08, skew=4)
    b = run_filter(ctx, x, head, taps, 9, 3, 2, SC08, skew=4)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_a_tap_beyond_two_signed_bytes_goes_to_the_generic_kernel(ctx, pool, monkeypatch):
    set_kernel(monkeypatch, "mfma")
    taps = np.array([32640, -100, 7, 32767], np.int16)
    check(ctx, pool[SC08][:3000], None, taps, 12, 1, 0, SC08)
    assert ctx.filter_last_plan()[0] == "generic"
    taps = np.array([32639, -100, 7, -32768], np.int16)
    check(ctx, pool[SC08][:3000], None, taps, 12, 1, 0, SC08)
    assert ctx.filter_last_plan()[0] == "mfma"


@pytest.mark.parametrize("kernel,in_size", [("generic", SC16), ("generic", SC08), ("mfma", SC08)])
def test_three_pieces_on_the_device_equal_one_call(ctx, pool, monkeypatch, kernel, in_size):
    """head points INTO the piece before, in the same device buffer; the phase is each piece's next_phase"""
    import torch
    set_kernel(monkeypatch, kernel)
    ntaps, decim, shift, nsamp = 65, 3, 13, 5003
    taps = taps_for(ntaps, "full")
    x = pool[in_size][:nsamp]
    sb = 2 * in_size                                                 # bytes of a sample
    src = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda()
    whole, wc = fr.filter_ref(x, None, taps, shift, decim, 1, SC16)
    dst = torch.full((4 * len(whole) + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    cuts = [0, 1700, 1700 + 1666, nsamp]                             # (multiples of 2 samples: an int8 head stays 4-byte aligned)
    phase, done, clipped = 1, 0, 0
    for lo, hi in zip(cuts, cuts[1:]):
        head = None if lo == 0 else src.data_ptr() + (lo - (ntaps - 1)) * sb
        n, c, _ = ctx.filter(hi - lo, in_size, src.data_ptr() + lo * sb, taps, shift, decim, phase, SC16, dst.data_ptr() + 4 * done, head_ptr=head)
        assert n == fr.span(hi - lo, decim, phase)[0]
        phase = fr.span(hi - lo, decim, phase)[1]
        done += n
        clipped += c
    got = dst.cpu().numpy()
    assert done == len(whole) and clipped == wc and (got[4 * done:] == GUARD).all()
    assert np.array_equal(got[:4 * done].view(np.int16).reshape(-1, 2), whole)


def test_refusals(ctx, monkeypatch):
    import torch
    set_kernel(monkeypatch, None)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    src, dst = buf.data_ptr(), buf.data_ptr() + (1 << 15)
    taps = np.array([1, 2, 1], np.int16)

    def call(nsamp=100, ss=SC08, src=src, head=None, taps=taps, shift=2, decim=2, phase=0, oss=SC08, dst=dst):
        return ctx.filter(nsamp, ss, src, taps, shift, decim, phase, oss, dst, head_ptr=head)

    def refused(code=-1, **kw):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))

    assert call()[0] == 50
    # each range limit from both sides
    big = np.zeros(513, np.int16)
    assert call(taps=big[:512])[0] == 50 and call(taps=big[:1])[0] == 50
    refused(taps=big)
    refused(taps=big[:0])
    assert call(decim=16, phase=15)[0] == 6 and call(decim=1)[0] == 100
    refused(decim=17)
    refused(decim=0)
    refused(phase=2)
    refused(phase=-1)
    assert call(shift=24)[0] == 50 and call(shift=0)[0] == 50
    refused(shift=25)
    refused(shift=-1)
    assert call(nsamp=0)[0] == 0
    refused(nsamp=-1)
    for ss in (0, 3, 4):
        refused(ss=ss)
        refused(oss=ss)
    # sum |taps| = 65535 passes, 65536 is GPSIQ_E_RANGE
    assert call(taps=np.array([32767, -32767, 1], np.int16))[0] == 50
    refused(code=-2, taps=np.array([32767, -32767, 2], np.int16))
    refused(code=-2, taps=np.array([-32768, -32768], np.int16))
    # pointers: alignment, NULL, overlap of the destination with the span and with the head
    refused(src=src + 2)
    refused(dst=dst + 2)
    refused(head=src + 1026)
    refused(src=None)
    refused(dst=None)
    refused(dst=src + 100)                                           # inside the span's 200 bytes
    assert call(src=src + 100, dst=src)[0] == 50                      # the destination's 100 bytes end where the span begins
    refused(src=src + 96, dst=src)
    refused(head=dst)                                                # the head's 4 bytes are the destination's first
    # a NULL nout, count and time are accepted
    assert gpsiq._filter(ctx._h, 100, SC08, src, None, gpsiq._p(taps), 3, 2, 2, 0, SC08, dst, None, None, None, None) == 0
