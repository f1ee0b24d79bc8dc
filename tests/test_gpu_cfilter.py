"""gpsiq_cfilter on the MI355X: every output byte, every guard byte and every count equals tests/_cfilter_ref.py's restatement of the
contract (include/gpsiq_rows.h, "Complex filter and notch"), on every kernel that can serve -- cfilter_generic, filter_mfma with
complex planes (int8 input), cfilter_mfma16 (int16 input) -- each forced through GPSIQ_CFILTER_KERNEL and confirmed with
gpsiq_cfilter_last_plan, whose plan is held to the planner's (tests/cfilter_plan.cpp).  Every destination lies between guard bytes
of 0x7f that must not change.  The shapes are the smallest at which a kernel can go wrong: both sides of a column (8 outputs), of a
wave's tile (128), of the runs a workgroup takes (256, 512, 1024), of the history, and spans that end before the first output; the
inputs are full-range, the extremes against taps at the sum bound, and values and tap entries on the byte seams of the digit and
stream planes.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import _cfilter_plan as cp
import _cfilter_ref as cr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

GUARD = 0x7F
PAD = 64                         # guard bytes either side of a destination
NTAPS = [1, 2, 16, 17, 33, 512]
SHAPES = [(1, 0), (3, 0), (3, 1), (3, 2), (16, 15)]                  # (decim, phase): every phase at decim 3
OUTPUTS = [127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
SHIFTS = [0, 14, 24]
MATRIX = {SC08: "mfma", SC16: "mfma16"}
SERVING = [("generic", SC08), ("generic", SC16), ("mfma", SC08), ("mfma", SC16)]
SEAMS16 = [-32768, -32513, -257, -256, -129, -128, -1, 0, 127, 128, 255, 256, 32639, 32640, 32767]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def pool(size):
    """full-range samples of a format every case cuts its span and head from (computed once, never written)"""
    p = cr.full_range(np.random.default_rng(770 + size), 40000, size)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def taps_for(ntaps, kind="mixed"):
    """mixed: both signs in both components, the sum well inside the range; full: sum |re| + |im| = 65535 exactly, every entry inside
    two signed bytes"""
    rng = np.random.default_rng(1000 * ntaps + len(kind))
    if kind == "mixed":
        lim = 60000 // (2 * ntaps) // 2 + 1
        t = rng.integers(-lim, lim + 1, size=(ntaps, 2))
        t[0] = (-3, 2)
    else:
        t = rng.integers(-20, 21, size=2 * ntaps).astype(np.int64)
        for k in range(2 * ntaps):
            add = min(65535 - int(np.abs(t).sum()), 32639 - abs(int(t[k])))
            t[k] += add * (1 if t[k] >= 0 else -1)
        t = t.reshape(-1, 2)
        assert int(np.abs(t).sum()) == (65535 if ntaps > 1 else 65278)
    t = t.astype(np.int16)
    t.setflags(write=False)
    return t


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_CFILTER_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_CFILTER_KERNEL", kernel)


def run_cfilter(ctx, x, head, taps, shift, decim, phase, out_size):
    """x [n, 2], head [ntaps - 1, 2] or None -> (out [nout, 2] as the device wrote it, clipped); guards compared"""
    import torch
    in_size = x.dtype.itemsize
    nsamp = len(x)
    nout = cr.span(nsamp, decim, phase)[0]
    raw = np.zeros(8 + x.nbytes, np.uint8)
    raw[:x.nbytes] = np.ascontiguousarray(x).view(np.uint8).ravel()
    src = torch.from_numpy(raw).cuda()
    hd = None if head is None or not len(head) else torch.from_numpy(np.ascontiguousarray(head).view(np.uint8).ravel().copy()).cuda()
    olen = 2 * nout * out_size
    dst = torch.full((2 * PAD + olen,), GUARD, dtype=torch.uint8, device="cuda")
    got_n, clipped, ms = ctx.cfilter(nsamp, in_size, src.data_ptr(), taps, shift, decim, phase, out_size, dst.data_ptr() + PAD,
                                     head_ptr=None if hd is None else hd.data_ptr())
    got = dst.cpu().numpy()
    assert got_n == nout and ms >= 0.0
    assert (got[:PAD] == GUARD).all() and (got[PAD + olen:] == GUARD).all(), "guard bytes of the destination changed"
    return got[PAD:PAD + olen].view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2).copy(), clipped


_refs = {}


def reference(key, x, head, taps, shift, decim, phase, out_size):
    """the restatement's answer, computed once per case and shared by the kernels that are held to it"""
    if key not in _refs:
        _refs[key] = cr.cfilter_ref(x, head, taps, shift, decim, phase, out_size)
    return _refs[key]


def check(ctx, x, head, taps, shift, decim, phase, out_size, key=None):
    want, wc = reference(key, x, head, taps, shift, decim, phase, out_size) if key else cr.cfilter_ref(x, head, taps, shift, decim, phase, out_size)
    got, gc = run_cfilter(ctx, x, head, taps, shift, decim, phase, out_size)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(x), len(taps), shift, decim, phase, "first differing output", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


def confirm(ctx, kernel, in_size, plan):
    """the last call took `kernel` (None: whatever the planner chose) with the planner's own grid, run and k-steps"""
    name, grid, run, steps = ctx.cfilter_last_plan()
    assert (name, grid, run, steps) == (cp.KERNELS[plan.kernel], plan.grid, plan.run, plan.steps)
    if kernel is not None:
        assert name == ("generic" if kernel == "generic" else MATRIX[in_size])


@pytest.mark.parametrize("ntaps", NTAPS)
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=["generic-int8", "generic-int16", "mfma-int8", "mfma16-int16"])
def test_sweep_of_taps_decimations_phases_and_lengths(ctx, monkeypatch, kernel, in_size, ntaps):
    set_kernel(monkeypatch, kernel)
    taps = taps_for(ntaps)
    cases = []
    for decim, phase in SHAPES:
        spans = {0, 1, max(ntaps - 1, 1), ntaps} | {phase + (n - 1) * decim + 1 for n in OUTPUTS}
        cases += [(decim, phase, nsamp) for nsamp in sorted(spans)]
    plans = cp.ask([("plan", n, in_size, ntaps, d, ph) + cp.stats(taps) + (cp.FORCE[kernel],) for d, ph, n in cases])
    for i, ((decim, phase, nsamp), plan) in enumerate(zip(cases, plans)):
        x = pool(in_size)[i:i + nsamp]
        head = None if i % 2 else pool(in_size)[30000 + i:30000 + i + ntaps - 1]
        out_size = (SC08, SC16)[(i // 2) % 2]
        check(ctx, x, head, taps, SHIFTS[i % 3], decim, phase, out_size, key=("sweep", in_size, ntaps, i))
        if isinstance(plan, cp.Nothing):                             # the span ends before its first output
            assert ctx.cfilter_last_plan()[0] is None and nsamp <= phase
            continue
        confirm(ctx, kernel, in_size, plan)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_the_int16_paths_reduced_runs(ctx, monkeypatch, kernel):
    """512 taps at decim 8 and 16: the two byte planes leave room for 512 and for 256 outputs a run; both sides of one and of two runs"""
    set_kernel(monkeypatch, kernel)
    taps = taps_for(512)
    for decim, run in ((8, 512), (16, 256)):
        plan = cp.plan(10 ** 5, SC16, 512, decim, 0, cp.stats(taps), cp.FORCE[kernel])
        assert kernel == "generic" or (plan.kernel, plan.run) == (cp.MFMA16, run)
        for nout in (run - 1, run, run + 1, 2 * run + 3):
            nsamp = (nout - 1) * decim + 1
            check(ctx, pool(SC16)[7:7 + nsamp], pool(SC16)[31000:31511], taps, 13, decim, 0, SC16, key=("reduced", decim, nout))
            confirm(ctx, kernel, SC16, cp.plan(nsamp, SC16, 512, decim, 0, cp.stats(taps), cp.FORCE[kernel]))


def test_the_default_is_the_planners(ctx, monkeypatch):
    set_kernel(monkeypatch, None)
    lim = cp.limits()
    for in_size, least in ((SC08, lim.min_taps8), (SC16, lim.min_taps16)):
        for ntaps in sorted({n for n in (1, least - 1, least, 512) if 1 <= n <= 512}):
            taps = taps_for(ntaps)
            check(ctx, pool(in_size)[:1500], None, taps, 10, 1, 0, SC16)
            confirm(ctx, None, in_size, cp.plan(1500, in_size, ntaps, 1, 0, cp.stats(taps), cp.AUTO))


def test_a_span_that_ends_before_the_first_output_writes_nothing(ctx, monkeypatch):
    set_kernel(monkeypatch, None)
    taps = taps_for(17)
    for decim, phase, nsamp in [(4, 3, 3), (4, 3, 2), (16, 15, 15), (16, 15, 1), (3, 2, 0), (1, 0, 0)]:
        got, clipped = run_cfilter(ctx, pool(SC16)[:nsamp], None, taps, 14, decim, phase, SC16)
        assert len(got) == 0 and clipped == 0 and ctx.cfilter_last_plan()[0] is None


@pytest.mark.parametrize("out_size", [SC08, SC16])
@pytest.mark.parametrize("kernel,in_size", SERVING, ids=["generic-int8", "generic-int16", "mfma-int8", "mfma16-int16"])
def test_format_pairs_shifts_and_a_clamp_that_fires(ctx, monkeypatch, kernel, in_size, out_size):
    """taps at the sum bound against a full-scale stream: at shift 0 nearly every element is clamped, at 24 none is, and the count is the
    restatement's (and so the same in both kernels); then the extremes alone, constant -128 / -32768 and +127 / +32767 against taps
    at the sum bound in all four sign patterns of (re, im): acc reaches -+(2^31 - 32768)"""
    set_kernel(monkeypatch, kernel)
    for ntaps, decim, phase, nsamp in [(17, 1, 0, 1500), (33, 3, 1, 3000), (512, 3, 1, 3000)]:
        taps = taps_for(ntaps, "full")
        counts = [check(ctx, pool(in_size)[5:5 + nsamp], pool(in_size)[20000:20000 + ntaps - 1], taps, shift, decim, phase, out_size,
                        key=("clamp", in_size, out_size, ntaps, shift)) for shift in SHIFTS]
        confirm(ctx, kernel, in_size, cp.plan(nsamp, in_size, ntaps, decim, phase, cp.stats(taps), cp.FORCE[kernel]))
        nel = 2 * cr.span(nsamp, decim, phase)[0]
        assert counts[0] > 0.9 * nel and counts[2] == 0, counts
    lo, hi = (-128, 127) if in_size == SC08 else (-32768, 32767)
    dt = pool(in_size).dtype
    for sre in (1, -1):
        for sim in (1, -1):
            taps = np.array([[sre * 4369, sim * 4369]] * 7 + [[sre * 4369, 0]], np.int16)     # 15 entries of 4369: the sum is 65535
            assert int(np.abs(taps.astype(np.int64)).sum()) == 65535
            for xi, xq in ((lo, lo), (hi, hi), (lo, hi), (hi, lo)):
                x = np.empty((300, 2), dt)
                x[:, 0], x[:, 1] = xi, xq
                for shift in (0, 16, 24):
                    check(ctx, x, x[:7], taps, shift, 2, 1, out_size, key=("extreme", in_size, out_size, sre, sim, xi, xq, shift))
    if in_size == SC16:
        # the accumulator's own limits: (re, im) = (-65535, 0) x -32768 = 2^31 - 32768 and its mirror, kept whole by shift 16 into int16
        taps = np.array([[-32767, 0], [-32767, 0], [-1, 0]], np.int16)
        x = np.full((200, 2), -32768, np.int16)
        check(ctx, x, x[:2], taps, 16, 1, 0, out_size)
        check(ctx, x, x[:2], -taps, 16, 1, 0, out_size)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_int16_values_on_the_byte_seams(ctx, monkeypatch, kernel):
    """every pair of seam values as (I, Q), and runs of one seam value, through taps that exercise both digit planes: a zero staged
    as 0x00 in the low plane, a wrong sign of the high byte or a carry between the planes shows here"""
    set_kernel(monkeypatch, kernel)
    s = np.array(SEAMS16, np.int16)
    pairs = np.array([(a, b) for a in s for b in s], np.int16)        # 225 samples
    x = np.concatenate([pairs, np.repeat(s, 40).reshape(-1, 1).repeat(2, axis=1), pairs[::-1]])
    for ntaps, decim in ((1, 1), (2, 1), (17, 3), (33, 1)):
        for kind in ("mixed", "full"):
            taps = taps_for(ntaps, kind)
            for head in (None, pairs[100:100 + ntaps - 1]):
                check(ctx, x, head, taps, 0 if kind == "mixed" and ntaps < 3 else 12, decim, 0, SC16,
                      key=("seams", ntaps, decim, kind, head is None))
                confirm(ctx, kernel, SC16, cp.plan(len(x), SC16, ntaps, decim, 0, cp.stats(taps), cp.FORCE[kernel]))
    # one tap of 1: the stream comes back as it went in, element for element (-32768 clamped to -32767, and counted)
    got, c = run_cfilter(ctx, x, None, np.array([[1, 0]], np.int16), 0, 1, 0, SC16)
    assert np.array_equal(got, np.maximum(x, -32767)) and c == int(np.count_nonzero(x == -32768))


@pytest.mark.parametrize("in_size", [SC08, SC16])
def test_tap_entries_on_the_digit_seams(ctx, monkeypatch, in_size):
    """+-127, +-128, +-32639 in re and im are served by the matrix kernels; 32640 in re or im, and im = -32768 (whose negative is
    no int16), fall to the generic kernel even when the matrix kernel is asked for; the bytes are the restatement's either way"""
    set_kernel(monkeypatch, "mfma")
    x = pool(in_size)[11:11 + 1200]
    head = pool(in_size)[25000:25003]
    served = [[[127, -127], [-128, 128], [128, -128], [-127, 127]], [[32639, 0], [0, -32639], [1, 127], [-128, -1]],
              [[0, 32639], [-32639, 0], [129, -128], [0, 0]], [[-32768, 5], [5, 127], [-128, 9], [0, 0]], [[255, -256], [256, -255], [-129, 129], [0, 0]]]
    fallen = [[[32640, 0], [0, 1], [2, 3], [4, 5]], [[0, 32640], [0, 1], [2, 3], [4, 5]], [[0, -32768], [0, 1], [2, 3], [4, 5]],
              [[0, -32640], [0, 1], [2, 3], [4, 5]]]
    for group, name in ((served, MATRIX[in_size]), (fallen, "generic")):
        for t in group:
            taps = np.array(t, np.int16)
            check(ctx, x, head, taps, 9, 1, 0, SC16)
            assert ctx.cfilter_last_plan()[0] == name, t


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=["generic-int8", "generic-int16", "mfma-int8", "mfma16-int16"])
def test_three_ragged_pieces_on_the_device_equal_one_call(ctx, monkeypatch, kernel, in_size):
    """head points INTO the piece before, in the same device buffer; the phase is each piece's next_phase"""
    import torch
    set_kernel(monkeypatch, kernel)
    ntaps, decim, shift, nsamp = 33, 3, 13, 3003
    taps = taps_for(ntaps, "full")
    x = pool(in_size)[:nsamp]
    sb = 2 * in_size                                                 # bytes of a sample
    src = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda()
    whole, wc = reference(("pieces", in_size), x, None, taps, shift, decim, 1, SC16)
    dst = torch.full((4 * len(whole) + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    cuts = [0, 1030, 1030 + 38, nsamp]                               # (multiples of 2 samples: an int8 head stays 4-byte aligned)
    phase, done, clipped = 1, 0, 0
    for lo, hi in zip(cuts, cuts[1:]):
        head = None if lo == 0 else src.data_ptr() + (lo - (ntaps - 1)) * sb
        n, c, _ = ctx.cfilter(hi - lo, in_size, src.data_ptr() + lo * sb, taps, shift, decim, phase, SC16, dst.data_ptr() + 4 * done, head_ptr=head)
        assert n == cr.span(hi - lo, decim, phase)[0]
        phase = cr.span(hi - lo, decim, phase)[1]
        done += n
        clipped += c
    got = dst.cpu().numpy()
    assert done == len(whole) and clipped == wc and (got[4 * done:] == GUARD).all()
    assert np.array_equal(got[:4 * done].view(np.int16).reshape(-1, 2), whole)


@pytest.mark.parametrize("kernel,in_size", SERVING, ids=["generic-int8", "generic-int16", "mfma-int8", "mfma16-int16"])
def test_the_two_identities_against_the_devices_own_filter(ctx, monkeypatch, kernel, in_size):
    import torch
    set_kernel(monkeypatch, kernel)
    nsamp, ntaps, decim, phase, shift = 2500, 33, 3, 2, 11
    x = pool(in_size)[40:40 + nsamp]
    head = pool(in_size)[26000:26000 + ntaps - 1]
    re = taps_for(ntaps)[:, 0].copy()
    src = torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda()
    hd = torch.from_numpy(np.ascontiguousarray(head).view(np.uint8).ravel().copy()).cuda()
    nout = cr.span(nsamp, decim, phase)[0]
    for out_size in (SC08, SC16):
        a = torch.full((2 * nout * out_size,), GUARD, dtype=torch.uint8, device="cuda")
        b = torch.full((2 * nout * out_size,), GUARD, dtype=torch.uint8, device="cuda")
        na, ca, _ = ctx.filter(nsamp, in_size, src.data_ptr(), re, shift, decim, phase, out_size, a.data_ptr(), head_ptr=hd.data_ptr())
        nb, cb, _ = ctx.cfilter(nsamp, in_size, src.data_ptr(), np.stack([re, np.zeros_like(re)], axis=1), shift, decim, phase, out_size, b.data_ptr(),
                                head_ptr=hd.data_ptr())
        assert (na, ca) == (nb, cb) and torch.equal(a, b)
        assert ctx.cfilter_last_plan()[0] == ("generic" if kernel == "generic" else MATRIX[in_size])
    # times j: (-Q, I)
    got, c = run_cfilter(ctx, x, None, np.array([[0, 1]], np.int16), 0, 1, 0, in_size)
    qmax = 127 if in_size == SC08 else 32767
    want = np.stack([-x[:, 1].astype(np.int64), x[:, 0].astype(np.int64)], axis=1)
    assert np.array_equal(got, np.clip(want, -qmax, qmax)) and c == int(np.count_nonzero(np.abs(want) > qmax))
    assert ctx.cfilter_last_plan()[0] == ("generic" if kernel == "generic" else MATRIX[in_size])


def test_refusals(ctx, monkeypatch):
    import torch
    set_kernel(monkeypatch, None)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    src, dst = buf.data_ptr(), buf.data_ptr() + (1 << 15)
    taps = np.array([[1, 0], [2, -1], [1, 1]], np.int16)

    def call(nsamp=100, ss=SC08, src=src, head=None, taps=taps, shift=2, decim=2, phase=0, oss=SC08, dst=dst):
        return ctx.cfilter(nsamp, ss, src, taps, shift, decim, phase, oss, dst, head_ptr=head)

    def refused(code=-1, **kw):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))

    assert call()[0] == 50
    # each range limit from both sides
    big = np.zeros((513, 2), np.int16)
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
    # sum |re| + |im| = 65535 passes, 65536 is GPSIQ_E_RANGE
    assert call(taps=np.array([[32767, -32767], [1, 0]], np.int16))[0] == 50
    refused(code=-2, taps=np.array([[32767, -32767], [1, 1]], np.int16))
    refused(code=-2, taps=np.array([[-32768, -32768]], np.int16))
    refused(code=-2, taps=np.array([[0, -32768], [0, 32767], [1, 0]], np.int16))
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
    assert gpsiq._cfilter(ctx._h, 100, SC08, src, None, gpsiq._p(taps), 3, 2, 2, 0, SC08, dst, None, None, None, None) == 0
