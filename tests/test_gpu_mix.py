"""gpsiq_mix on the MI355X: every output byte, every guard byte and every count equals tests/_mix_ref.py's restatement of the contract
(include/gpsiq_rows.h, "Mix"), on both kernels (GPSIQ_MIX_KERNEL) and on the default path, whose choice is held to the planner's
(tests/mix_plan.cpp).  The sources are random full-range elements, each followed on the device by poison the contract says is never
read, and every destination lies between guard bytes of 0x7f that must not change.  The shapes are the smallest at which a kernel can
go wrong: both sides of a 16-byte slot, of a wave and of a workgroup, every misalignment of destination and source against each
other, delays on each side of a slot and of the span, sweeps and gates shorter and longer than a slot.  Run with -m gpu."""
import numpy as np
import pytest

import _mix_plan as mp
import _mix_ref as mr
import gpsiq
from gpsiq.abi import MIX_ROTATED, MIX_STREAM, MIX_TONE, SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
POISON = 0x5A
PAD = 64                         # guard bytes either side of a destination, poison bytes behind a source
NSAMP = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 257, 4099]
OFFSETS = [0, 4, 8, 12]
KERNELS = ["generic", "rows", None]
IDS = ["generic", "rows", "default"]
FORCE = {"generic": mp.GENERIC, "rows": mp.ROWS, None: mp.AUTO}
DTYPE = {SC08: np.int8, SC16: np.int16}
E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """full-range samples of either format every case cuts its sources from (computed once, never written)"""
    rng = np.random.default_rng(91)
    p = {ss: mr.full_range(rng, 6000, ss) for ss in (SC08, SC16)}
    for a in p.values():
        a.setflags(write=False)
    return p


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_MIX_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_MIX_KERNEL", kernel)


def stream(pool, kind, ss, gain, nsamp, skip=0, at=0, off=0, **kw):
    """a stream term that holds exactly the samples the contract reads, its device copy `off` bytes past a 16-byte boundary"""
    t = mr.Term(kind, gain, pool[ss][at:at + max(0, nsamp - skip)], skip=skip, **kw)
    t.off = off
    return t


def run_mix(ctx, nsamp, m0, terms, shift, qmax, out_size, dst_off=0, inplace=None, kernel=None):
    """-> (out [nsamp, 2] as the device wrote it, clipped); guards compared.  inplace: the index of the term whose source is dst"""
    import torch
    olen = 2 * nsamp * out_size
    dst = torch.full((2 * PAD + dst_off + olen,), GUARD, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    at = PAD + dst_off
    keep, mts = [], []
    for k, t in enumerate(terms):
        if t.x is None:
            mts.append(t.mixterm())
        elif k == inplace:
            assert t.skip == 0 and t.sample_size == out_size and len(t.x) == nsamp
            dst[at:at + olen] = torch.from_numpy(np.ascontiguousarray(t.x).view(np.uint8).ravel().copy()).cuda()
            mts.append(t.mixterm(dst.data_ptr() + at))
        else:
            off = getattr(t, "off", 0)
            raw = np.full(off + t.x.nbytes + PAD, POISON, np.uint8)
            raw[off:off + t.x.nbytes] = np.ascontiguousarray(t.x).view(np.uint8).ravel()
            src = torch.from_numpy(raw).cuda()
            assert src.data_ptr() % 16 == 0
            keep.append(src)
            mts.append(t.mixterm(src.data_ptr() + off))
    clipped, ms = ctx.mix(nsamp, m0, mts, shift, qmax, out_size, dst.data_ptr() + at)
    got = dst.cpu().numpy()
    assert ms >= 0.0
    assert (got[:at] == GUARD).all() and (got[at + olen:] == GUARD).all(), "guard bytes of the destination changed"
    plan = mp.plan(nsamp, m0, out_size, dst.data_ptr() + at, FORCE[kernel])
    assert ctx.mix_last_plan()[:3] == ((None, 0, 0) if plan is None else (mp.KERNELS[plan.kernel], plan.grid, plan.units))
    return got[at:at + olen].view(DTYPE[out_size]).reshape(-1, 2).copy(), clipped


def check(ctx, nsamp, m0, terms, shift, qmax, out_size, dst_off=0, inplace=None, kernel=None):
    want, wc = mr.mix_ref(nsamp, m0, terms, shift, qmax, DTYPE[out_size])
    got, gc = run_mix(ctx, nsamp, m0, terms, shift, qmax, out_size, dst_off, inplace, kernel)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (nsamp, m0, shift, qmax, out_size, dst_off, "first differing sample", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
@pytest.mark.parametrize("out_size", [SC08, SC16])
def test_lengths_and_destination_offsets(ctx, pool, monkeypatch, kernel, out_size):
    """every length at every offset of the destination, with all three kinds, both source formats, a delay, a sweep and a gate"""
    set_kernel(monkeypatch, kernel)
    clipped = 0
    for i, nsamp in enumerate(NSAMP):
        for j, doff in enumerate(OFFSETS):
            terms = [stream(pool, MIX_STREAM, SC08, 150, nsamp, off=OFFSETS[(i + j) % 4], at=i),
                     stream(pool, MIX_ROTATED, SC16, -2, nsamp, skip=(3, 1, 64, 0)[j], off=OFFSETS[(i + 2 * j + 1) % 4], step=(11 << 50) + 777, rate=-(1 << 46),
                            sweep=(65, 7), at=j),
                     mr.Term(MIX_TONE, 40, phase0=5 << 55, step=-(37 << 50), gate=(3, 1, 2)),
                     mr.Term(MIX_TONE, -25, step=1 << 52, rate=1 << 49, sweep=(7, 3), gate=(129, 64, 100))]
            clipped += check(ctx, nsamp, 1000 + i, terms, 8, 127 if out_size == SC08 else 20000, out_size, doff, kernel=kernel)
    assert clipped > 0


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
@pytest.mark.parametrize("in_size,out_size", [(SC08, SC08), (SC08, SC16), (SC16, SC08), (SC16, SC16)])
def test_format_pairs_delays_and_every_misalignment(ctx, pool, monkeypatch, kernel, in_size, out_size):
    """one stream term of either kind: every delay on each side of a slot and of the span, at every pair of source and destination
    offsets (the delay shifts the source's alignment too)"""
    set_kernel(monkeypatch, kernel)
    shift, qmax = (0, 32767) if out_size == SC16 and in_size == SC08 else (9, 127 if out_size == SC08 else 32767)
    case = 0
    for nsamp in (9, 65, 257):
        for skip in sorted({0, 1, 3, 64, nsamp - 1, nsamp, nsamp + 5}):
            for kind in (MIX_STREAM, MIX_ROTATED):
                gain = (1 << shift) + 3 if kind == MIX_STREAM else 2 if shift else 1
                t = stream(pool, kind, in_size, gain, nsamp, skip=skip, off=OFFSETS[case % 4], at=case, step=-(3 << 50) + case, phase0=case << 52)
                check(ctx, nsamp, 7, [t], shift, qmax, out_size, OFFSETS[(case // 4) % 4], kernel=kernel)
                case += 1
    for soff in OFFSETS:                                               # and all sixteen pairs at one shape
        for doff in OFFSETS:
            for skip in (0, 1, 2):
                t = stream(pool, MIX_ROTATED, in_size, 2 if shift else 1, 263, skip=skip, off=soff, step=(200 << 50) + 1)
                check(ctx, 263, 0, [t, mr.Term(MIX_TONE, 1, step=5 << 50)], shift, qmax, out_size, doff, kernel=kernel)


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
def test_sweeps_gates_signs_and_far_indices(ctx, pool, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    for m0, nsamp in ((2 ** 32 - 2000, 4099), (2 ** 40 + 1, 4099), (2 ** 40 + 1, 65), (0, 257)):
        for period in (2, 5, 7, 64, 65):
            for offset in sorted({0, 1, period - 1}):
                for sign in (1, -1):
                    terms = [mr.Term(MIX_TONE, sign * 100, phase0=3 << 57, step=sign * ((29 << 50) + 12345), rate=-sign * ((1 << 47) + 99), sweep=(period, offset)),
                             stream(pool, MIX_ROTATED, SC08, -sign, nsamp, skip=2, off=4, step=-sign * (1 << 51), rate=sign * (1 << 48), sweep=(period, offset),
                                    gate=(3, 1, offset % 3)),
                             mr.Term(MIX_TONE, 50, step=1 << 40, rate=sign * 5, gate=(129, 64, 128 - offset))]
                    check(ctx, nsamp, m0, terms, 4, 32767, SC16, 8, kernel=kernel)
            if nsamp == 4099 and period > 5:
                break                                                  # the far indices: three periods are enough at the long span
    # a rate without a restart: r is the absolute index itself
    check(ctx, 4099, 2 ** 40 + 1, [mr.Term(MIX_TONE, 100, step=-(1 << 56), rate=(1 << 20) + 1)], 0, 32767, SC16, kernel=kernel)
    # an index past 2^63: m + offset may wrap, the plan sends every such span to the generic kernel
    terms = [mr.Term(MIX_TONE, 100, step=(1 << 50) + 1, rate=3, sweep=(7, 6), gate=(5, 2, 4))]
    check(ctx, 65, 2 ** 64 - 30, terms, 0, 127, SC08, kernel=kernel)
    assert ctx.mix_last_plan()[0] == "generic"


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
@pytest.mark.parametrize("out_size", [SC08, SC16])
def test_eight_terms(ctx, pool, monkeypatch, kernel, out_size):
    set_kernel(monkeypatch, kernel)
    for nsamp, doff in ((257, 4), (4099, 0)):
        terms = []
        for k in range(8):
            kind = (MIX_STREAM, MIX_ROTATED, MIX_TONE)[k % 3]
            kw = dict(step=(k + 1) * (17 << 50) * (-1) ** k, phase0=k << 56, rate=k << 44, sweep=((0, 0), (64, 5), (65, 64), (7, 0))[k % 4],
                      gate=((0, 0, 0), (3, 1, 0), (129, 64, 3))[k % 3])
            if kind == MIX_TONE:
                terms.append(mr.Term(kind, 30 - 9 * k, **kw))
            else:
                if kind == MIX_STREAM:
                    kw = dict(gate=kw["gate"])
                terms.append(stream(pool, kind, (SC08, SC16)[k % 2], (100, -1)[k % 2] * (k + 1), nsamp, skip=(0, 1, 5, 300)[k % 4], off=OFFSETS[k % 4],
                                    at=100 * k, **kw))
        check(ctx, nsamp, 12345, terms, 10, 127 if out_size == SC08 else 32767, out_size, doff, kernel=kernel)


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
@pytest.mark.parametrize("in_size,out_size,qmax", [(SC08, SC08, 1), (SC08, SC08, 7), (SC08, SC08, 127), (SC16, SC16, 32767), (SC16, SC08, 127),
                                                   (SC16, SC16, 1), (SC08, SC16, 7)])
def test_the_count_is_exact_at_full_scale(ctx, pool, monkeypatch, kernel, in_size, out_size, qmax):
    """full-scale inputs at shift 0: -128 and -32768 are the only elements a clamp at the format's own qmax changes"""
    set_kernel(monkeypatch, kernel)
    rng = np.random.default_rng(3)
    lo, hi = (-128, 127) if in_size == SC08 else (-32768, 32767)
    x = rng.choice(np.array([lo, lo + 1, -1, 0, 1, hi], DTYPE[in_size]), size=(1031, 2))
    t = mr.Term(MIX_STREAM, 1, x)
    t.off = 4
    clipped = check(ctx, 1031, 0, [t], 0, qmax, out_size, 12, kernel=kernel)
    assert clipped == int(np.count_nonzero(np.abs(x.astype(np.int64)) > qmax)) and clipped > 0


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
@pytest.mark.parametrize("size", [SC08, SC16])
def test_in_place(ctx, pool, monkeypatch, kernel, size):
    """dst is the stream term's own source: a tone and a delayed copy of ANOTHER buffer are added where the stream lies"""
    set_kernel(monkeypatch, kernel)
    for nsamp in (1, 7, 8, 9, 65, 257, 4099):
        for doff in OFFSETS:
            terms = [mr.Term(MIX_TONE, 33, step=19 << 50, rate=1 << 45, sweep=(64, 1)),
                     stream(pool, MIX_STREAM, size, 1 << 6, nsamp, at=doff),
                     stream(pool, MIX_ROTATED, size, 1, nsamp, skip=3, off=(doff + 4) % 16, at=500, step=-(5 << 50))]
            check(ctx, nsamp, 99, terms, 6, 127 if size == SC08 else 32767, size, doff, inplace=1, kernel=kernel)
    # the same source twice, as it is and turned, both in place
    x = pool[size][:777]
    terms = [mr.Term(MIX_STREAM, 1 << 8, x), mr.Term(MIX_ROTATED, 1, x, step=128 << 50)]
    want, wc = mr.mix_ref(777, 0, terms, 8, 127 if size == SC08 else 32767, DTYPE[size])
    import torch
    buf = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda()
    gc, _ = ctx.mix(777, 0, [t.mixterm(buf.data_ptr()) for t in terms], 8, 127 if size == SC08 else 32767, size, buf.data_ptr())
    assert np.array_equal(buf.cpu().numpy().view(DTYPE[size]).reshape(-1, 2), want) and gc == wc


@pytest.mark.parametrize("kernel", KERNELS, ids=IDS)
def test_two_calls_give_the_same_bytes(ctx, pool, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    terms = [stream(pool, MIX_STREAM, SC16, 3, 4099, skip=1, off=8), mr.Term(MIX_TONE, 1000, step=3 << 50, rate=1 << 40, sweep=(65, 0), gate=(129, 64, 0))]
    a = run_mix(ctx, 4099, 5, terms, 2, 127, SC08, 4, kernel=kernel)
    b = run_mix(ctx, 4099, 5, terms, 2, 127, SC08, 4, kernel=kernel)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_refusals(ctx, monkeypatch):
    import torch
    monkeypatch.delenv("GPSIQ_MIX_KERNEL", raising=False)
    n = 64
    src = torch.zeros(4 * n + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((4 * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    S, D = src.data_ptr(), dst.data_ptr()
    T = gpsiq.MixTerm
    good = T.stream(S, SC16, 1)

    def refused(terms, nsamp=n, shift=0, qmax=127, out=SC08, ptr=D):
        with pytest.raises(gpsiq.GpsiqError) as e:
            ctx.mix(nsamp, 0, terms, shift, qmax, out, ptr)
        assert e.value.code == E_ARG, e.value

    ctx.mix(n, 0, [good], 0, 127, SC08, D)                            # the shape the refusals below each break in one place
    refused([])
    refused([good] * 9)
    refused([good], nsamp=-1)
    refused([good], shift=-1)
    refused([good], shift=41)
    refused([good], qmax=0)
    refused([good], qmax=128)
    refused([good], qmax=32768, out=SC16)
    refused([good], out=3)
    refused([good], ptr=0)
    refused([good], ptr=D + 2)
    refused([T(kind=3, gain=1)])
    refused([T.stream(0, SC16, 1)])
    refused([T.stream(S + 2, SC16, 1)])
    refused([T.stream(S, 3, 1)])
    refused([T.stream(S, SC16, 1, gate=(3, 4, 0))])
    refused([T.stream(S, SC16, 1, gate=(3, 1, 3))])
    refused([T.stream(S, SC16, 1, gate=(0, 0, 1))])
    refused([T.tone(1, 1, sweep=(5, 5))])
    refused([T.tone(1, 1, sweep=(0, 1))])
    for field in ("reserved", "reserved2"):
        t = T.tone(1, 1)
        setattr(t, field, 1)
        refused([t])
    t = T.tone(1, 1)
    t.src = S
    refused([t])
    t = T.tone(1, 1)
    t.skip = 1
    refused([t])
    # overlap: a delayed term on dst, a term of another format on dst, a term that starts inside dst, dst that starts inside a term
    refused([T.stream(D, SC08, 1, skip=1)])
    refused([T.stream(D, SC16, 1)])
    refused([T.stream(D + 4, SC08, 1)])
    refused([T.stream(D - 4, SC08, 1)], ptr=D)
    refused([T.rotated(D, SC08, 1, 1 << 50, skip=n - 1)])
    ctx.mix(n, 0, [T.stream(D, SC08, 1), T.rotated(D, SC08, 1, 1 << 50)], 0, 127, SC08, D)      # in place, twice: allowed
    ctx.mix(n, 0, [T.stream(D, SC08, 1, skip=n)], 0, 127, SC08, D)                              # nothing of it is read: no overlap
    ctx.mix(n, 0, [T.stream(D + 2 * n, SC08, 1)], 0, 127, SC08, D)                              # back to back
    assert (dst.cpu().numpy()[4 * n:] == GUARD).all()
    # nothing is launched for an empty span, and the count is 0
    assert ctx.mix(0, 0, [good], 0, 127, SC08, D)[0] == 0 and ctx.mix_last_plan()[0] is None
