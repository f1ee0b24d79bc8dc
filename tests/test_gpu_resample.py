"""gpsiq_resample on the MI355X: every output byte, every guard byte, every count and every next position equals tests/_resample_ref.py's
restatement of the contract (include/gpsiq_rows.h, "Resample"), on both kernels (GPSIQ_RESAMPLE_KERNEL) and on the default path, whose
choice is held to the planner's (tests/resample_plan.cpp).  The spans are random full-range elements -- the kernels are pure functions
of the stream -- every source and head ends in poison bytes and every destination lies between guard bytes of 0x7f that must not
change.  The shapes are the smallest at which a kernel can go wrong: both sides of a wave, of a workgroup, of a run of outputs and of
the history, every step at which the position arithmetic changes character, and spans that end before the first output.
Run with -m gpu."""
import numpy as np
import pytest

import _resample_plan as rp
import _resample_ref as rr
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

ONE = 1 << 32
GUARD = 0x7F
POISON = 0xA5                    # behind every source and head: 0xA5A5 as a sample would not go unnoticed
PAD = 64                         # guard bytes either side of a destination
STEPS = [ONE, ONE + 1, ONE - 1, 1 << 29, 1 << 35, 3 << 31, round(ONE * 2.6 / 2.048), round(ONE * (1 + 20e-6)), 0x16A09E667]
FORCE = {"generic": rp.GENERIC, "rows": rp.ROWS, None: rp.AUTO}
KERNEL_PARAMS = pytest.mark.parametrize("kernel", ["generic", "rows", None], ids=["generic", "rows", "default"])


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
    rng = np.random.default_rng(78)
    p = {ss: rr.full_range(rng, 600000, ss) for ss in (SC08, SC16)}
    for a in p.values():
        a.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def limits():
    return rp.limits()


def table(L, ntaps, seed=0, total=None):
    return rr.random_table(np.random.default_rng(1000 * L + ntaps + seed), L, ntaps, total)


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_RESAMPLE_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_RESAMPLE_KERNEL", kernel)


def device_bytes(a, skew):
    """the bytes of array a on the device, `skew` bytes past a 16-byte boundary, poison before and behind -> (tensor, pointer)"""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).ravel()
    raw = np.full(16 + len(b) + 64, POISON, np.uint8)
    raw[skew:skew + len(b)] = b
    t = torch.from_numpy(raw).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + skew


def run_resample(ctx, x, head, taps, L, shift, interp, step, pos0, out_size, skew=(0, 0, 0)):
    """x [n, 2], head [ntaps - 1, 2] or None -> (out [nout, 2] as the device wrote it, clipped, next_pos); guards compared.  skew: bytes
    the span, the head and the destination start past a 16-byte boundary"""
    import torch
    in_size = x.dtype.itemsize
    nsamp = len(x)
    nout, nxt = rr.span(nsamp, pos0, step)
    src, src_ptr = device_bytes(x, skew[0])
    hd, hd_ptr = (None, None) if head is None or not len(head) else device_bytes(head, skew[1])
    olen = 2 * nout * out_size
    dst = torch.full((2 * PAD + 16 + olen,), GUARD, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    lead = PAD + skew[2]
    got_n, got_next, clipped, ms = ctx.resample(nsamp, in_size, src_ptr, taps, L, shift, interp, step, pos0, out_size, dst.data_ptr() + lead, head_ptr=hd_ptr)
    got = dst.cpu().numpy()
    assert (got_n, got_next) == (nout, nxt) and ms >= 0.0
    assert (got[:lead] == GUARD).all() and (got[lead + olen:] == GUARD).all(), "guard bytes of the destination changed"
    del src, hd
    return got[lead:lead + olen].copy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2), clipped, got_next


def check(ctx, x, head, taps, L, shift, interp, step, pos0, out_size, skew=(0, 0, 0)):
    want, wc, _, _ = rr.resample_ref(x, head, taps, L, shift, interp, step, pos0, out_size)
    got, gc, _ = run_resample(ctx, x, head, taps, L, shift, interp, step, pos0, out_size, skew)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert not len(bad), (len(x), np.shape(taps), shift, interp, step, pos0, "first differing output", int(bad[0]), got[bad[0]], want[bad[0]])
    assert gc == wc
    return gc


def confirm_plan(ctx, kernel, nsamp, L, ntaps, step, pos0):
    """the plumbing entry names the kernel that ran, its grid and its unit: the planner's, and the forced kernel where one was forced"""
    plan = rp.plan(nsamp, L, ntaps, step, pos0, FORCE[kernel])
    name, grid, run, pieces = ctx.resample_last_plan()
    if isinstance(plan, rp.Nothing):
        assert name is None
        return
    assert (name, grid, run, pieces) == (rp.KERNELS[plan.kernel], plan.grid, plan.run, 0)
    if kernel is not None:
        assert name == kernel


def shape_for(target, step, k):
    """(nsamp, pos0) of a span with exactly `target` outputs at `step`; its last output lies `slack` short of the span's end, slack
    walking through the step with k (0: the last fraction, phase nphases - 1 with mu 255)"""
    slack = (k * (step // 4 + 12345)) % step
    nsamp = -(-((target - 1) * step + 1 + slack) // ONE)
    pos0 = nsamp * ONE - (target - 1) * step - 1 - slack
    assert rr.span(nsamp, pos0, step)[0] == target
    return nsamp, pos0


@KERNEL_PARAMS
def test_output_counts_either_side_of_wave_workgroup_and_run_at_every_step(ctx, pool, limits, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    L, ntaps = 5, 7
    taps = table(L, ntaps)
    run = limits.run
    targets = [1, 63, 64, 65, 255, 256, 257, run - 1, run, run + 1, 2 * run + 1]
    i = 0
    for step in STEPS:
        for target in targets:
            nsamp, pos0 = shape_for(target, step, i)
            x = pool[SC08][i:i + nsamp]
            head = None if i % 2 else pool[SC08][500000 + i:500000 + i + ntaps - 1]
            check(ctx, x, head, taps, L, (0, 9, 16)[i % 3], (i // 2) % 2, step, pos0, SC08)
            if target in (run, 2 * run + 1):
                confirm_plan(ctx, kernel, nsamp, L, ntaps, step, pos0)
            i += 1


@KERNEL_PARAMS
def test_span_lengths_around_the_history_and_positions(ctx, pool, monkeypatch, kernel):
    """nsamp 0, 1, ntaps - 2, ntaps - 1, ntaps; pos0 0, 2^32 - 1 (last phase, mu 255, row nphases read), 2^31 and at or past the span's end"""
    set_kernel(monkeypatch, kernel)
    L, ntaps = 4, 9
    taps = table(L, ntaps)
    i = 0
    for step in (ONE, 1 << 29, 1 << 35, STEPS[6]):
        for nsamp in (0, 1, ntaps - 2, ntaps - 1, ntaps):
            for pos0 in (0, ONE - 1, 1 << 31, nsamp * ONE, nsamp * ONE + 5 * ONE + 3):
                x = pool[SC16][i:i + nsamp]
                head = None if i % 3 == 0 else pool[SC16][400000 + i:400000 + i + ntaps - 1]
                got, clipped, nxt = run_resample(ctx, x, head, taps, L, 7, i % 2, step, pos0, SC16)
                want, wc, wn, wnext = rr.resample_ref(x, head, taps, L, 7, i % 2, step, pos0, SC16)
                assert np.array_equal(got, want) and clipped == wc and nxt == wnext
                if pos0 >= nsamp * ONE:
                    assert len(got) == 0 and clipped == 0 and nxt == pos0 - nsamp * ONE and ctx.resample_last_plan()[0] is None
                confirm_plan(ctx, kernel, nsamp, L, ntaps, step, pos0)
                i += 1


@KERNEL_PARAMS
@pytest.mark.parametrize("L,ntaps", [(0, 1), (0, 16), (1, 2), (5, 7), (8, 1), (8, 2), (8, 7), (8, 16), (8, 32), (6, 64)])
def test_table_shapes(ctx, pool, monkeypatch, kernel, L, ntaps):
    """every row count and tap count, odd and even, the largest tables; with and without interp, also with a single phase"""
    set_kernel(monkeypatch, kernel)
    taps = table(L, ntaps, total=65535 if ntaps > 2 else None)
    i = 0
    for step in (STEPS[6], ONE - 1, 1 << 35, 1 << 29):
        nsamp = 700 if step >= ONE - 1 else 90
        for interp in (0, 1):
            x, head = pool[SC08][i:i + nsamp], pool[SC08][300000 + i:300000 + i + ntaps - 1]
            check(ctx, x, head, taps, L, (14, 16)[interp], interp, step, (ONE - 1, 1 << 31)[i % 2], SC16)
            i += 1
    confirm_plan(ctx, kernel, nsamp, L, ntaps, step, (ONE - 1, 1 << 31)[(i - 1) % 2])


@KERNEL_PARAMS
@pytest.mark.parametrize("in_size,out_size", [(SC08, SC08), (SC08, SC16), (SC16, SC08), (SC16, SC16)])
def test_format_pairs_at_the_accumulators_edge(ctx, monkeypatch, kernel, in_size, out_size):
    """full-scale inputs against rows whose absolute sum is 65535: all of one sign against the most negative value (|a| = 65535 * 32768,
    the largest the contract allows), and alternating signs against a stream that alternates with them, neighbouring rows starting on
    opposite signs, so that a0 and a1 sit at opposite ends and the 64-bit combine carries the whole range; shifts 0, 8 and 16"""
    set_kernel(monkeypatch, kernel)
    lo, hi = (-128, 127) if in_size == SC08 else (-32768, 32767)
    dt = np.int8 if in_size == SC08 else np.int16
    L, ntaps = 3, 15
    alt = rr.alternating_table(L, ntaps)
    neg = -np.abs(alt)
    n = 400
    const = np.full((n, 2), lo, dt)
    swing = np.where((np.arange(n) % 2 == 0)[:, None], lo, hi).astype(dt).repeat(2, axis=1).reshape(n, 2)
    swing[:, 1] = np.where(np.arange(n) % 2 == 0, hi, lo)            # Q the other way round
    counts = []
    for taps, x in ((neg, const), (alt, swing), (alt, const)):
        for shift in (0, 8, 16):
            for interp in (0, 1):
                for step in (ONE, ONE + (1 << 27), 3 << 31):
                    counts.append(check(ctx, x, x[:ntaps - 1], taps, L, shift, interp, step, 0, out_size))
    assert counts[0] > 0                                             # the clamp fires at shift 0 ...
    if out_size == SC16:
        assert min(counts) == 0                                      # ... and rests at 16, where alternating taps meet a constant stream
    # the edge itself, by hand: 15 taps of -4369 against the most negative value, shift 0: a0 = 65535 * |lo|, clamped
    got, clipped, _ = run_resample(ctx, const[:20], const[:14], np.full((2, 15), -4369, np.int16), 0, 0, 1, ONE, 0, out_size)
    assert (got == (127 if out_size == SC08 else 32767)).all() and clipped == 40
    if in_size == SC16 and out_size == SC16:                          # shift 16: (65535 * 32768 + 2^15) >> 16 = 32768 -> 32767, clamped by one
        got, clipped, _ = run_resample(ctx, const[:20], const[:14], np.full((2, 15), -4369, np.int16), 0, 16, 0, ONE, 0, out_size)
        assert (got == 32767).all() and clipped == 40


def test_exact_counts_at_qmax(ctx, monkeypatch):
    """one tap of 1, shift 0: values at qmax pass uncounted, one beyond is clamped and counted -- expected by hand"""
    for kernel in ("generic", "rows"):
        set_kernel(monkeypatch, kernel)
        x = np.array([[126, 127], [128, -127], [-128, -129], [0, 32767]], np.int16)
        got, clipped, _ = run_resample(ctx, x, None, np.array([[1], [1]], np.int16), 0, 0, 0, ONE, 0, SC08)
        assert got.tolist() == [[126, 127], [127, -127], [-127, -127], [0, 127]] and clipped == 4
        x = np.array([[16383, 16384], [-16383, -16384]], np.int16)       # times 2: 32766, 32768 | -32766, -32768
        for interp in (0, 1):
            got, clipped, _ = run_resample(ctx, x, None, np.array([[2], [2]], np.int16), 0, 0, interp, ONE, 0, SC16)
            assert got.tolist() == [[32766, 32767], [-32766, -32767]] and clipped == 2


@pytest.mark.parametrize("kernel", ["generic", "rows"])
@pytest.mark.parametrize("interp", [0, 1])
def test_identity_table_gives_the_input_delayed(ctx, pool, monkeypatch, kernel, interp):
    """step 2^32, pos0 0, one phase, a single tap of 2^shift: the expected bytes are the input's own"""
    set_kernel(monkeypatch, kernel)
    shift, ntaps, delay = 9, 7, 3
    x = pool[SC16][1000:2200].copy()
    x[x == -32768] = -32767
    rows = np.zeros((2, ntaps), np.int16)
    rows[0, delay] = rows[1, delay - 1] = 1 << shift
    got, clipped, nxt = run_resample(ctx, x, None, rows, 0, shift, interp, ONE, 0, SC16)
    assert clipped == 0 and nxt == 0 and np.array_equal(got, np.concatenate([np.zeros((delay, 2), np.int16), x[:len(x) - delay]]))


@pytest.mark.parametrize("kernel", ["generic", "rows"])
@pytest.mark.parametrize("in_size", [SC08, SC16])
def test_every_alignment_of_source_head_and_destination(ctx, pool, monkeypatch, kernel, in_size):
    """each of the three at 0, 4, 8 and 12 bytes past a 16-byte boundary, the head given and not; poison behind source and head"""
    set_kernel(monkeypatch, kernel)
    L, ntaps = 5, 16
    taps = table(L, ntaps)
    x, head = pool[in_size][77:77 + 1333], pool[in_size][9000:9000 + ntaps - 1]
    i = 0
    for s in (0, 4, 8, 12):
        for h in (0, 4, 8, 12):
            d = (s + 2 * h + 4 * (i % 3)) % 16
            check(ctx, x, head if i % 4 else None, taps, L, 12, i % 2, (STEPS[6], 1 << 34, 1 << 30)[i % 3], ONE - 1, (SC08, SC16)[i % 2], skew=(s, h, d))
            i += 1
    for d in (0, 4, 8, 12):
        check(ctx, x, head, taps, L, 12, 1, STEPS[6], 0, SC08, skew=(4, 12, d))


@pytest.mark.parametrize("kernel", ["generic", "rows"])
def test_the_same_call_twice(ctx, pool, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    taps = table(7, 16, total=65535)
    x, head = pool[SC08][100:100 + 2777], pool[SC08][9000:9015]
    a = run_resample(ctx, x, head, taps, 7, 9, 1, STEPS[6], 12345, SC08, skew=(4, 4, 4))
    b = run_resample(ctx, x, head, taps, 7, 9, 1, STEPS[6], 12345, SC08, skew=(4, 4, 4))
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] > 0


@KERNEL_PARAMS
def test_more_units_than_the_grid_cap(ctx, pool, limits, monkeypatch, kernel):
    """every workgroup strides over several units: the outputs past grid * unit"""
    set_kernel(monkeypatch, kernel)
    L, ntaps, step = 5, 7, ONE + 1
    nsamp = limits.run * limits.max_grid + 2 * limits.run + 17
    assert nsamp <= 600000
    check(ctx, pool[SC08][:nsamp], None, table(L, ntaps), L, 9, 1, step, 0, SC08)
    name, grid, run, _ = ctx.resample_last_plan()
    plan = rp.plan(nsamp, L, ntaps, step, 0, FORCE[kernel])
    assert (name, grid, run) == (rp.KERNELS[plan.kernel], limits.max_grid, plan.run) and plan.runs > limits.max_grid


@pytest.mark.parametrize("kernel", ["generic", "rows"])
@pytest.mark.parametrize("in_size,step", [(SC16, STEPS[6]), (SC08, 1 << 35), (SC08, 1 << 29), (SC16, STEPS[7])])
def test_pieces_on_the_device_equal_one_call(ctx, pool, limits, monkeypatch, kernel, in_size, step):
    """splits at 1, ntaps - 2, ntaps - 1 and at the edge of a run; three pieces behind the split, of which one is shorter than the history
    and, at the steps above two samples an output, gives no output; head is the ntaps - 1 samples before the piece, from more than one
    earlier piece where those are short; pos0 is the piece before's next_pos"""
    import torch
    set_kernel(monkeypatch, kernel)
    L, ntaps, shift, pos0 = 6, 16, 13, ONE - 1
    taps = table(L, ntaps, total=65535)
    run_edge = ((limits.run * step + pos0) >> 32) + 1                # the first sample whose outputs belong to the second run
    nsamp = run_edge + 700
    x = pool[in_size][:nsamp]
    whole, wc, wn, wnext = rr.resample_ref(x, None, taps, L, shift, 1, step, pos0, SC16)
    hist = np.concatenate([np.zeros((ntaps - 1, 2), x.dtype), x])    # hist[lo : lo + ntaps - 1] are the samples before sample lo
    empty = 0
    for cut in (1, ntaps - 2, ntaps - 1, run_edge):
        cuts = [0, cut, cut + 300, cut + 303, nsamp]
        dst = torch.full((4 * wn + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        pos, done, clipped = pos0, 0, 0
        for lo, hi in zip(cuts, cuts[1:]):
            piece, piece_ptr = device_bytes(x[lo:hi], 4)
            head, head_ptr = device_bytes(hist[lo:lo + ntaps - 1], 8)
            n, nxt, c, _ = ctx.resample(hi - lo, in_size, piece_ptr, taps, L, shift, 1, step, pos, SC16, dst.data_ptr() + 4 * done,
                                        head_ptr=None if lo == 0 else head_ptr)
            assert (n, nxt) == rr.span(hi - lo, pos, step)
            empty += n == 0
            pos, done, clipped = nxt, done + n, clipped + c
        got = dst.cpu().numpy()
        assert done == wn and pos == wnext and clipped == wc and (got[4 * done:] == GUARD).all()
        assert np.array_equal(got[:4 * done].view(np.int16).reshape(-1, 2), whole), cut
    if step >= 1 << 34:
        assert empty > 0


def test_refusals(ctx, monkeypatch):
    import torch
    set_kernel(monkeypatch, None)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    src, dst = buf.data_ptr(), buf.data_ptr() + (1 << 15)
    taps = np.zeros((3, 3), np.int16)
    taps[:, 1] = 4

    def call(nsamp=100, ss=SC08, src=src, head=None, taps=taps, L=1, shift=2, interp=1, step=2 * ONE, pos0=0, oss=SC08, dst=dst):
        return ctx.resample(nsamp, ss, src, taps, L, shift, interp, step, pos0, oss, dst, head_ptr=head)

    def refused(code=-1, **kw):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == code, (kw, str(e.value))

    assert call()[:2] == (50, 0)
    # each range limit from both sides
    assert call(L=0, taps=np.zeros((2, 3), np.int16))[0] == 50 and call(L=8, taps=np.zeros((257, 3), np.int16))[0] == 50
    refused(L=-1)
    refused(L=9, taps=np.zeros((513, 3), np.int16))
    assert call(taps=np.zeros((3, 1), np.int16))[0] == 50 and call(taps=np.zeros((3, 64), np.int16))[0] == 50
    refused(taps=np.zeros((3, 65), np.int16))
    refused(taps=np.zeros((3, 0), np.int16))
    assert call(L=7, taps=np.zeros((129, 64), np.int16))[0] == 50     # 8256 entries
    refused(L=8, taps=np.zeros((257, 33), np.int16))                  # 8481
    refused(L=8, taps=np.zeros((257, 64), np.int16))
    assert call(shift=16)[0] == 50 and call(shift=0)[0] == 50
    refused(shift=17)
    refused(shift=-1)
    assert call(interp=0)[0] == 50
    refused(interp=2)
    refused(interp=-1)
    assert call(step=1 << 29)[0] == 800 and call(step=1 << 35)[0] == 13
    refused(step=(1 << 29) - 1)
    refused(step=(1 << 35) + 1)
    refused(step=0)
    assert call(pos0=(1 << 63) - 1)[:2] == (0, (1 << 63) - 1 - 100 * ONE)
    refused(pos0=1 << 63)
    assert call(nsamp=0)[:2] == (0, 0)
    refused(nsamp=-1)
    for ss in (0, 3, 4):
        refused(ss=ss)
        refused(oss=ss)
    # sum |taps| of a row: 65535 passes, 65536 is GPSIQ_E_RANGE -- in any row, the last included, with interp or without
    ok = np.zeros((3, 3), np.int16)
    ok[:] = [32767, -32767, 1]
    assert call(taps=ok)[0] == 50
    for r in range(3):
        bad = ok.copy()
        bad[r, 2] = 2
        refused(code=-2, taps=bad)
        refused(code=-2, taps=bad, interp=0)
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
    # a NULL count, position, clip count and time are accepted
    assert gpsiq._resample(ctx._h, 100, SC08, src, None, gpsiq._p(taps), 1, 3, 2, 1, 2 * ONE, 0, SC08, dst, None, None, None, None, None) == 0
