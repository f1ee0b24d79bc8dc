"""Stream order and wide offsets of gpsiq_array_cov / gpsiq_array_combine on the MI355X (include/gpsiq_rows.h, "Array").
Stream order as tests/test_gpu_stage_streams.py has it for the other stages (its fillers, its side stream and its two conditions are
used as they are): the buffer the stage reads holds 0x7f until a producer queued on a side stream behind a long filler puts the true
input there; the stage is called on that stream at once and must return the restatement's answer for the true input.  Before each
ordered call the same context makes an ordinary call on the 0x7f bytes, so that its scratch and its counter hold the answer to the
wrong input.  Wide offsets: two int16 streams of 2^30 + 5000 samples each, whose byte offsets pass 2^32, through both calls; the
streams are not periodic in 2^32 bytes, so a 32-bit offset reads other samples.  Run with -m gpu."""
import numpy as np
import pytest

import _array_ref as ar
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import copy_producer, guarded, ordered, scratch, side  # noqa: F401  (scratch and side are fixtures)

pytestmark = pytest.mark.gpu

NSAMP = 30011


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def staged_elements(in_size, nelem):
    """(the streams, their bytes back to back on the device, the byte offset of every element: each a multiple of 16)"""
    import torch
    xs = ar.streams(np.random.default_rng(600 + in_size), nelem, NSAMP, in_size)
    step = -(-xs[0].nbytes // 16) * 16
    raw = np.zeros(step * nelem, np.uint8)
    for e, x in enumerate(xs):
        raw[e * step:e * step + x.nbytes] = x.view(np.uint8).ravel()
    return xs, torch.from_numpy(raw).cuda(), [e * step for e in range(nelem)]


@pytest.mark.parametrize("kernel,in_size", [("generic", SC08), ("generic", SC16), ("mfma", SC08)], ids=["generic-int8", "generic-int16", "mfma-int8"])
def test_covariance_waits_for_its_producer(ctx, scratch, side, monkeypatch, kernel, in_size):  # noqa: F811
    monkeypatch.setenv("GPSIQ_ARRAY_KERNEL", kernel)
    xs, staged, at = staged_elements(in_size, 3)
    buf = guarded(staged)
    ptrs = [buf.data_ptr() + a for a in at]
    want = ar.cov_ref(xs)
    wrong, _ = ctx.array_cov(ptrs, NSAMP, in_size)                     # the answer to the 0x7f bytes: what the scratch holds now
    assert not np.array_equal(wrong, want)
    got, _ = ordered(scratch, side, copy_producer(buf, staged), lambda s: ctx.array_cov(ptrs, NSAMP, in_size, stream=s))
    assert ctx.array_last_plan()[0] == kernel
    assert np.array_equal(got, want)


@pytest.mark.parametrize("in_size,out_size", [(SC08, SC16), (SC16, SC08)], ids=["8to16", "16to8"])
def test_combiner_waits_for_its_producer(ctx, scratch, side, in_size, out_size):  # noqa: F811
    import torch
    xs, staged, at = staged_elements(in_size, 3)
    buf = guarded(staged)
    ptrs = [buf.data_ptr() + a for a in at]
    w = np.array([[900, -300], [-1200, 40], [5, 2000]], np.int16)
    shift = 4 if in_size == SC08 else 19                               # some elements clamp, most do not
    want, wc = ar.combine_ref(xs, w, shift, out_size)
    assert 0 < wc < want.size // 2
    dst = torch.zeros(2 * NSAMP * out_size, dtype=torch.uint8, device="cuda")
    wrong = ctx.array_combine(ptrs, NSAMP, in_size, w, shift, out_size, dst.data_ptr())[0]
    assert wrong != wc                                                 # the counter holds the answer to the wrong input
    clipped, _ = ordered(scratch, side, copy_producer(buf, staged), lambda s: ctx.array_combine(ptrs, NSAMP, in_size, w, shift, out_size, dst.data_ptr(), stream=s))
    got = dst.cpu().numpy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2)
    assert np.array_equal(got, want) and clipped == wc


# ---- wide offsets ---------------------------------------------------------------------------------------------------------------------
WIDE = 2 ** 30 + 5000
TILE = 1 << 20
NEED = 2 * 4 * WIDE + 2 * WIDE + (3 << 30)                             # two int16 streams, an int8 output, and room to work in


@pytest.fixture(scope="module")
def wide():
    """two int16 streams of WIDE samples on the device: tile k of 2^20 samples is a fixed random tile plus (stream 0) or minus
    (stream 1) k in both components, wrapping in int16 -- every tile differs from every other, so no offset that is wrong by a multiple of
    anything reads the right samples"""
    import torch
    free, total = torch.cuda.mem_get_info()
    assert free >= NEED, "the wide-offset tests need %.1f GiB of free device memory, %.1f of %.1f GiB are free" % (NEED / 2 ** 30, free / 2 ** 30, total / 2 ** 30)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2030)
    tiles = [torch.randint(-32768, 32768, (2 * TILE,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(2)]
    xs = [torch.empty(2 * WIDE, dtype=torch.int16, device="cuda") for _ in range(2)]
    for k in range(-(-WIDE // TILE)):
        lo, hi = 2 * k * TILE, min(2 * (k + 1) * TILE, 2 * WIDE)
        xs[0][lo:hi] = tiles[0][:hi - lo] + k
        xs[1][lo:hi] = tiles[1][:hi - lo] - k
    torch.cuda.synchronize()
    yield xs
    del xs
    torch.cuda.empty_cache()


def test_covariance_past_4_gib(ctx, wide):
    """against the restatement computed in chunks of 2^22 samples with torch's int64 arithmetic on the device (nothing of the library)"""
    import torch
    got, _ = ctx.array_cov([x.data_ptr() for x in wide], WIDE, SC16)
    want = torch.zeros((2, 2, 2), dtype=torch.int64, device="cuda")
    chunk = 1 << 22
    for lo in range(0, WIDE, chunk):
        part = [x[2 * lo:2 * min(lo + chunk, WIDE)].view(-1, 2).to(torch.int64) for x in wide]
        i = torch.stack([p[:, 0] for p in part])
        q = torch.stack([p[:, 1] for p in part])
        for a in range(2):
            for b in range(2):
                want[a, b, 0] += (i[a] * i[b] + q[a] * q[b]).sum()
                want[a, b, 1] += (q[a] * i[b] - i[a] * q[b]).sum()
    want = want.cpu().numpy()
    # the chunks' own arithmetic, on the last 5000 samples through numpy
    tail = [x[2 * (WIDE - 5000):].cpu().numpy().reshape(-1, 2) for x in wide]
    part = [x[2 * (WIDE - 5000):].view(-1, 2).to(torch.int64) for x in wide]
    assert int((part[0][:, 1] * part[1][:, 0] - part[0][:, 0] * part[1][:, 1]).sum()) == int(ar.cov_ref(tail)[0, 1, 1])
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


def test_combiner_past_4_gib(ctx, wide):
    """the bytes at the very end, the bytes either side of the sources' byte offset 2^32, and the count of the whole span"""
    import torch
    w = np.array([[3000, -1000], [-500, 2500]], np.int16)
    shift = 20                                                         # |acc| <= 7000 * 32768 = 2^27.8: about one output in twenty clamps at +-127
    dst = torch.full((2 * WIDE + 128,), 0x7F, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.array_combine([x.data_ptr() for x in wide], WIDE, SC16, w, shift, SC08, dst.data_ptr() + 64)
    assert (dst[:64] == 0x7F).all() and (dst[64 + 2 * WIDE:] == 0x7F).all()
    total = 0
    for lo, hi in ((WIDE - 6000, WIDE), (2 ** 30 - 3000, 2 ** 30 + 3000), (0, 3000)):
        xs = [x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2) for x in wide]
        want, _ = ar.combine_ref(xs, w, shift, SC08)
        got = dst[64 + 2 * lo:64 + 2 * hi].cpu().numpy().view(np.int8).reshape(-1, 2)
        assert np.array_equal(got, want), (lo, hi)
    # the count, from the restatement's own steps in chunks on the device
    chunk = 1 << 22
    for lo in range(0, WIDE, chunk):
        part = [x[2 * lo:2 * min(lo + chunk, WIDE)].view(-1, 2).to(torch.int64) for x in wide]
        acc_i = sum(int(w[e, 0]) * part[e][:, 0] - int(w[e, 1]) * part[e][:, 1] for e in range(2))
        acc_q = sum(int(w[e, 0]) * part[e][:, 1] + int(w[e, 1]) * part[e][:, 0] for e in range(2))
        for acc in (acc_i, acc_q):
            y = (acc + (1 << (shift - 1))) >> shift
            total += int(((y > 127) | (y < -127)).sum())
    assert clipped == total and total > 0
