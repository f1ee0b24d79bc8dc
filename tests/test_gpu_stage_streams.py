"""Stream order of the five stream stages on the MI355X: "the kernels are queued on hip_stream ... behind the caller's gpsiq_launch on
that stream" (include/gpsiq_rows.h).  Every other stage test passes the null stream, where a step queued on the wrong stream cannot
show.  Here the buffer a stage reads holds 0x7f until a producer queued on a SIDE stream -- behind a filler of some tens of
milliseconds, so that it has certainly not run when the stage is called -- puts the true input there; the stage is called on that
stream at once and must return the cached reference of the true input, byte for byte.  Before each ordered call the same context
makes an ordinary call of the same shape on the 0x7f bytes, so that what its buffers hold is the answer to the wrong input
(tests/test_stage_contract_cases.py: different from the expected one in every case) and a copy-back cannot pass by luck.

A step that waits for nothing -- a memset of the sums, the upload of the states -- does no harm by running EARLY on another stream, so
the null stream, where such a slip would most likely put it, is kept busy as well, by a filler four times as long queued first: there the
step runs LATE, behind everything the call queued on the side stream, the kernel adds into the sums or continues from the states the
ordinary call left, and the result is wrong.  A kernel, a relaunch or a copy-back on the null stream then also runs behind the call's
own later steps.  Each case asserts both conditions itself: the producer has not run when the stage is called, and the null stream is
still busy when it returns.  Run with -m gpu."""
import time

import numpy as np
import pytest

import _contract_cases as cc
import gpsiq
from gpsiq.abi import SC16
from test_gpu_acquire import same as same_search
from test_gpu_acquire import to_device as span_to_device
from test_gpu_follow import same as same_follow

pytestmark = pytest.mark.gpu

GUARD = cc.GUARD
# The fillers: in-place adds of 1 over one half of a scratch tensor each, FILLER_ADDS on the side stream in front of the producer and
# NULL_FILLER times as many on the null stream, queued first (the two share the memory system while both run).  The side filler's
# device time is to be 20 times the host time from its first queued add to the stage call or more; the margin is for a busy shared host.
# Measured once on the MI355X over the 16 cases (every case prints its figures): 0.26 to 0.36 ms on the host from the first queued add
# to the stage call, 58.7 to 59.4 ms of side filler on the device (160 times and more), and the null stream's filler ended 82.1 to
# 82.4 ms behind the producer, where the longest stage call (the 64-block launch and its despread) needs some 23 ms.
FILLER_BYTES = 1 << 32
FILLER_ADDS = 40
NULL_FILLER = 4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scratch():
    """(the side filler's half, the null filler's half)"""
    import torch
    t = torch.zeros(FILLER_BYTES, dtype=torch.uint8, device="cuda")
    warm = torch.cuda.Stream()
    with torch.cuda.stream(warm):                 # the first add, copy and event load their kernels: not inside a measured case
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(warm)
        t[:FILLER_BYTES // 2].add_(1)
        t[:16].copy_(t[16:32])
    torch.cuda.synchronize()
    yield t[:FILLER_BYTES // 2], t[FILLER_BYTES // 2:]
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def side(scratch):
    """A side stream that runs BESIDE the null stream.  A process has few hardware queues (four by default) and the runtime deals its
    streams out over them when they are first used: one that shares the null stream's queue runs behind the null stream's filler,
    which is another experiment.  Streams are tried until the work of one finishes while the null stream is still busy."""
    import torch
    for _ in range(32):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        for _ in range(8):
            scratch[1].add_(1)
        null_done, mine = torch.cuda.Event(), torch.cuda.Event()
        null_done.record(torch.cuda.default_stream())
        with torch.cuda.stream(s):
            scratch[0][:1 << 20].add_(1)
            mine.record(s)
        mine.synchronize()
        beside = not null_done.query()
        torch.cuda.synchronize()
        if beside:
            return s
    pytest.fail("no side stream ran beside the null stream: 32 streams all waited for its filler")


def ordered(scratch, side, produce, stage):
    """the null stream's filler; then filler, producer and an event on the side stream with nothing in between; then stage(side stream),
    called while the producer has not run and returning while the null stream is busy -> what the stage returned"""
    import torch
    torch.cuda.synchronize()
    start, mid, done, null_done = (torch.cuda.Event(enable_timing=True) for _ in range(4))
    for _ in range(NULL_FILLER * FILLER_ADDS):
        scratch[1].add_(1)
    null_done.record(torch.cuda.default_stream())
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        start.record(side)
        for _ in range(FILLER_ADDS):
            scratch[0].add_(1)
        mid.record(side)
        produce(side)
        done.record(side)
    pending = not done.query()
    host_ms = 1e3 * (time.perf_counter() - t0)
    assert pending, "the producer had finished before the stage was called (%.3f ms after queueing began): the case proves nothing" % host_ms
    out = stage(side.cuda_stream)
    busy = not null_done.query()
    call_ms = 1e3 * (time.perf_counter() - t0) - host_ms
    assert busy, "the null stream had drained before the stage returned (%.3f ms): a step queued there by mistake would not have shown" % call_ms
    torch.cuda.synchronize()
    print("queueing to stage call %.3f ms on the host, side filler %.3f ms on the device, producer %.3f ms, stage call %.3f ms, null filler ended %.3f ms behind the producer"
          % (host_ms, start.elapsed_time(mid), mid.elapsed_time(done), call_ms, done.elapsed_time(null_done)))
    return out


def guarded(staged):
    """a device tensor of staged's size and alignment, every byte 0x7f"""
    import torch
    buf = torch.full_like(staged, GUARD)
    assert buf.data_ptr() % 16 == staged.data_ptr() % 16
    return buf


def copy_producer(buf, staged):
    return lambda side: buf.copy_(staged)


# ---- despread -----------------------------------------------------------------------------------------------------------------------

def same_despread(got, ref):
    for g, r, what in zip(got[:3], ref, ("sums", "prn", "stats")):
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), what


@pytest.mark.parametrize("name", cc.STREAM_DESPREAD)
def test_despread_behind_a_copy(ctx, scratch, side, name, monkeypatch):
    from test_gpu_despread import to_device
    import _despread_plan as dp
    c, q, stream, ref = cc.despread_reference(name)
    for k, v in dp.case_env(c).items():
        monkeypatch.setenv(k, v)
    ctx.set_descriptors(q)
    staged, stride = to_device(stream, c.guard)
    assert stride % 4 == 0
    buf = guarded(staged)
    call = lambda s: ctx.despread(c.block0, c.nblocks, c.nsamp, c.ss, buf.data_ptr(), stride, c.seg_len, clip=cc.DESPREAD_CLIP[c.ss], stream=s)
    wrong = call(None)
    assert wrong[0].tobytes() != ref[0].tobytes() and wrong[2].tobytes() != ref[2].tobytes()
    got = ordered(scratch, side, copy_producer(buf, staged), call)
    assert ctx.despread_last_plan()[0] == c.kernel
    same_despread(got, ref)
    assert bytes(buf.cpu().numpy()) == bytes(staged.cpu().numpy())


def test_despread_behind_the_launch_that_renders_its_stream(ctx, scratch, side):
    """the header's own sentence: gpsiq_launch of the closed loop's 64 blocks on the side stream, the noise on, and gpsiq_despread on
    that stream at once -- the sums of tests/test_despread_ref.py's loop, and the stream it rendered"""
    import torch
    import _despread_ref as dr
    from test_despread_ref import loop_reference
    L = dr.LOOP
    q, ref_stream, ref_sums, ref_prn = loop_reference()
    stride = 4 * L["nsamp"]
    buf = torch.full((L["nblocks"] * stride,), GUARD, dtype=torch.uint8, device="cuda")
    ctx.set_noise(L["seed"], gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"]), 0)
    try:
        ctx.set_descriptors(q)
        call = lambda s: ctx.despread(0, L["nblocks"], L["nsamp"], SC16, buf.data_ptr(), stride, L["seg_len"], clip=32767, stream=s)
        ctx.launch(0, 1, L["nsamp"], SC16, buf.data_ptr(), stride)            # the first launch of a shape loads its kernel
        ctx.synchronize()
        buf.fill_(GUARD)
        wrong = call(None)
        assert wrong[0].tobytes() != ref_sums.tobytes()
        got = ordered(scratch, side, lambda side: ctx.launch(0, L["nblocks"], L["nsamp"], SC16, buf.data_ptr(), stride, stream=side.cuda_stream), call)
        assert got[0].tobytes() == ref_sums.tobytes() and np.array_equal(got[1], ref_prn)
        assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(L["nblocks"], -1), ref_stream)
        assert np.array_equal(got[2], dr.stats(ref_stream, L["nsamp"], 32767))
    finally:
        ctx.noise_off()


# ---- pack, unpack -------------------------------------------------------------------------------------------------------------------

def up4(n):
    return (n + 3) & ~3


def rows(blocks, stride, tail=0):
    """blocks: uint8 [nblocks][len] -> device uint8 [nblocks * stride + tail], 0x7f wherever no block byte lies"""
    import torch
    buf = np.full(len(blocks) * stride + tail, GUARD, dtype=np.uint8)
    buf[:len(blocks) * stride].reshape(len(blocks), stride)[:, :blocks.shape[1]] = blocks
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("ss,bits", cc.PACK_FORMATS, ids=lambda v: str(v))
def test_pack_behind_a_copy(ctx, scratch, side, ss, bits):
    import torch
    x, want, count, _ = cc.pack_reference(ss, bits)
    nb, n = cc.STREAM_PACK_BLOCKS, cc.STREAM_PACK_NSAMP
    sstride, dstride = up4(2 * n * ss) + 4, up4(want.shape[1]) + 4
    staged = rows(np.ascontiguousarray(x).view(np.uint8).reshape(nb, -1), sstride)
    src = guarded(staged)
    dst, other = (torch.full((nb * dstride + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2))
    wrong = ctx.pack(nb, n, ss, src.data_ptr(), sstride, bits, other.data_ptr(), dstride)
    assert wrong[0] == cc.pack_of_guard(ss, bits)[1] != count
    clipped, _ = ordered(scratch, side, copy_producer(src, staged), lambda s: ctx.pack(nb, n, ss, src.data_ptr(), sstride, bits, dst.data_ptr(), dstride, stream=s))
    assert clipped == count
    assert bytes(dst.cpu().numpy()) == bytes(rows(want, dstride, 64).cpu().numpy())


@pytest.mark.parametrize("ss,bits", cc.PACK_FORMATS, ids=lambda v: str(v))
def test_unpack_behind_a_copy(ctx, scratch, side, ss, bits):
    import torch
    _, packed, _, want = cc.pack_reference(ss, bits)
    nb, n = cc.STREAM_PACK_BLOCKS, cc.STREAM_PACK_NSAMP
    sstride, dstride = up4(packed.shape[1]) + 4, up4(2 * n * ss) + 4
    staged = rows(packed, sstride)
    src = guarded(staged)
    dst, other = (torch.full((nb * dstride + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2))
    ctx.unpack(nb, n, bits, src.data_ptr(), sstride, ss, other.data_ptr(), dstride)
    ordered(scratch, side, copy_producer(src, staged), lambda s: ctx.unpack(nb, n, bits, src.data_ptr(), sstride, ss, dst.data_ptr(), dstride, stream=s))
    assert bytes(dst.cpu().numpy()) == bytes(rows(np.ascontiguousarray(want).view(np.uint8).reshape(nb, -1), dstride, 64).cpu().numpy())


# ---- acquire ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["mfma", "generic"])
@pytest.mark.parametrize("name", cc.STREAM_ACQUIRE)
def test_acquire_behind_a_copy(ctx, scratch, side, name, kernel, monkeypatch):
    import _acquire_plan as ap
    monkeypatch.setenv("GPSIQ_ACQUIRE_KERNEL", kernel)
    c = cc.by_name(ap.CASES, name)
    stream, steps, ref = cc.acquire_reference(name)
    nsamp = len(stream) // 2
    staged, ptr = span_to_device(stream, c.base, c.guard)
    buf = guarded(staged)
    at = buf.data_ptr() + (ptr - staged.data_ptr())
    call = lambda s: ctx.acquire(nsamp, c.ss, at, c.prns, *steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop, stream=s, corr=True)
    wrong = call(None)
    assert all(w.tobytes() != r.tobytes() for w, r in zip(wrong[:3], ref))
    got = ordered(scratch, side, copy_producer(buf, staged), call)
    assert ctx.acquire_last_plan()[0] == kernel
    same_search(got, ref)


# ---- follow -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.STREAM_FOLLOW)
def test_follow_behind_a_copy_with_relaunches(ctx, scratch, side, name, monkeypatch):
    from test_gpu_follow import to_device
    monkeypatch.setenv("GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH", str(cc.STREAM_FOLLOW_KNOB))
    c, stream, cfg, states, ref = cc.follow_reference(name)
    nsamp = len(stream) // 2
    staged, ptr = to_device(stream, c.base, c.guard)
    buf = guarded(staged)
    at = buf.data_ptr() + (ptr - staged.data_ptr())
    call = lambda s: ctx.follow(nsamp, c.ss, at, cfg, states, c.max_epochs, stream=s)
    wrong = call(None)
    assert wrong[0].tobytes() != ref[0].tobytes() and wrong[2].tobytes() != ref[2].tobytes()
    got = ordered(scratch, side, copy_producer(buf, staged), call)
    assert ctx.follow_last_plan()[2] == int(max(ref[1])) // cc.STREAM_FOLLOW_KNOB + 1 > 2
    same_follow(got, ref)
