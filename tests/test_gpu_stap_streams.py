"""Stream order and wide offsets of gpsiq_stap_cov / gpsiq_stap_combine on the MI355X (include/gpsiq_rows.h, "Space-time array").
Stream order as tests/test_gpu_array_streams.py has it for the array (the fillers, the side stream and the two conditions of
tests/test_gpu_stage_streams.py are used as they are): the buffer the stage reads -- streams and heads -- holds 0x7f until a producer
queued on a side stream behind a long filler puts the true input there; the stage is called on that stream at once and must return
the restatement's answer for the true input.  Before each ordered call the same context makes an ordinary call on the 0x7f bytes, so
that its scratch and its counter hold the answer to the wrong input.  Wide offsets: two int16 streams of 2^29 + 5000 samples each,
whose byte offsets pass 2^31, through both calls; the streams are not periodic in 2^31 bytes, so a 32-bit offset reads other samples.
Run with -m gpu."""
import numpy as np
import pytest

import _stap_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import copy_producer, guarded, ordered, scratch, side  # noqa: F401  (scratch and side are fixtures)

pytestmark = pytest.mark.gpu

NSAMP = 30011
NELEM, NTAPS = 3, 4


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def staged_elements(in_size):
    """(the streams, their heads, the bytes of both back to back on the device, the byte offsets of the streams and of the heads: each
    a multiple of 16)"""
    import torch
    pool = sr.streams(np.random.default_rng(700 + in_size), NELEM, NSAMP + NTAPS - 1, in_size)
    xs, heads = [x[NTAPS - 1:] for x in pool], sr.heads_of(pool, NTAPS - 1, NTAPS)
    step = -(-xs[0].nbytes // 16) * 16
    raw = np.zeros((step + 16) * NELEM, np.uint8)
    at, hat = [], []
    for e, (x, h) in enumerate(zip(xs, heads)):
        at.append(e * step)
        hat.append(NELEM * step + 16 * e)
        raw[at[e]:at[e] + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).ravel()
        raw[hat[e]:hat[e] + h.nbytes] = np.ascontiguousarray(h).view(np.uint8).ravel()
    return xs, heads, torch.from_numpy(raw).cuda(), at, hat


@pytest.mark.parametrize("kernel,in_size", [("generic", SC08), ("generic", SC16), ("mfma", SC08)], ids=["generic-int8", "generic-int16", "mfma-int8"])
def test_covariance_waits_for_its_producer(ctx, scratch, side, monkeypatch, kernel, in_size):  # noqa: F811
    monkeypatch.setenv("GPSIQ_STAP_KERNEL", kernel)
    xs, heads, staged, at, hat = staged_elements(in_size)
    buf = guarded(staged)
    ptrs, hptrs = [buf.data_ptr() + a for a in at], [buf.data_ptr() + a for a in hat]
    want = sr.cov_ref(xs, heads, NTAPS)
    wrong, _ = ctx.stap_cov(ptrs, NSAMP, in_size, NTAPS, heads=hptrs)   # the answer to the 0x7f bytes: what the scratch holds now
    assert not np.array_equal(wrong, want)
    got, _ = ordered(scratch, side, copy_producer(buf, staged), lambda s: ctx.stap_cov(ptrs, NSAMP, in_size, NTAPS, heads=hptrs, stream=s))
    assert ctx.stap_last_plan()[0] == kernel
    assert np.array_equal(got, want)


@pytest.mark.parametrize("in_size,out_size", [(SC08, SC16), (SC16, SC08)], ids=["8to16", "16to8"])
def test_combiner_waits_for_its_producer(ctx, scratch, side, in_size, out_size):  # noqa: F811
    import torch
    xs, heads, staged, at, hat = staged_elements(in_size)
    buf = guarded(staged)
    ptrs, hptrs = [buf.data_ptr() + a for a in at], [buf.data_ptr() + a for a in hat]
    w = np.random.default_rng(8).integers(-700, 701, size=(NELEM, NTAPS, 2)).astype(np.int16)
    shift = 3 if in_size == SC08 else 19                               # some elements clamp, most do not
    want, wc = sr.combine_ref(xs, heads, w, shift, out_size)
    assert 0 < wc < want.size // 2
    dst = torch.zeros(2 * NSAMP * out_size, dtype=torch.uint8, device="cuda")
    wrong = ctx.stap_combine(ptrs, NSAMP, in_size, w, shift, out_size, dst.data_ptr(), heads=hptrs)[0]
    assert wrong != wc                                                 # the counter holds the answer to the wrong input
    clipped, _ = ordered(scratch, side, copy_producer(buf, staged),
                         lambda s: ctx.stap_combine(ptrs, NSAMP, in_size, w, shift, out_size, dst.data_ptr(), heads=hptrs, stream=s))
    got = dst.cpu().numpy().view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2)
    assert np.array_equal(got, want) and clipped == wc


# ---- wide offsets ---------------------------------------------------------------------------------------------------------------------
WIDE = 2 ** 29 + 5000
TILE = 1 << 20
WTAPS = 2
NEED = 2 * 4 * WIDE + 2 * WIDE + (3 << 30)                             # two int16 streams, an int8 output, and room to work in


def test_both_calls_past_2_gib(ctx):
    """Two int16 streams of WIDE samples: tile k of 2^20 samples is a fixed random tile plus (stream 0) or minus (stream 1) k in both
    components, wrapping in int16 -- every tile differs from every other.  Two taps, heads of one sample.  The covariance against the
    restatement computed in chunks of 2^22 samples with torch's int64 arithmetic on the device (nothing of the library), that
    arithmetic itself held to numpy on the last 5000 samples; the combiner's bytes at the very end, at the start (where the heads
    are read) and either side of the sources' byte offset 2^31, and its count over the whole span."""
    import torch
    free, total = torch.cuda.mem_get_info()
    assert free >= NEED, "the wide-offset test needs %.1f GiB of free device memory, %.1f of %.1f GiB are free" % (NEED / 2 ** 30, free / 2 ** 30, total / 2 ** 30)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2031)
    tiles = [torch.randint(-32768, 32768, (2 * TILE,), dtype=torch.int16, device="cuda", generator=gen) for _ in range(2)]
    wide = [torch.empty(2 * WIDE, dtype=torch.int16, device="cuda") for _ in range(2)]
    for k in range(-(-WIDE // TILE)):
        lo, hi = 2 * k * TILE, min(2 * (k + 1) * TILE, 2 * WIDE)
        wide[0][lo:hi] = tiles[0][:hi - lo] + k
        wide[1][lo:hi] = tiles[1][:hi - lo] - k
    heads_np = [np.array([[1234, -4321]], np.int16), np.array([[-777, 31000]], np.int16)]
    heads = [torch.from_numpy(h.ravel().copy()).cuda() for h in heads_np]
    torch.cuda.synchronize()
    ptrs, hptrs = [x.data_ptr() for x in wide], [h.data_ptr() for h in heads]

    def rows_of(lo, hi):
        """the four rows' I and Q over samples [lo, hi) as int64 on the device: row 2 e + t is x_e(n - t)"""
        out = []
        for e in range(2):
            now = wide[e][2 * lo:2 * hi].view(-1, 2).to(torch.int64)
            first = heads[e].view(1, 2).to(torch.int64) if lo == 0 else wide[e][2 * (lo - 1):2 * lo].view(1, 2).to(torch.int64)
            out += [now, torch.cat([first, now[:-1]])]
        return out

    got, _ = ctx.stap_cov(ptrs, WIDE, SC16, WTAPS, heads=hptrs)
    want = torch.zeros((4, 4, 2), dtype=torch.int64, device="cuda")
    chunk = 1 << 22
    for lo in range(0, WIDE, chunk):
        z = rows_of(lo, min(lo + chunk, WIDE))
        i = torch.stack([r[:, 0] for r in z])
        q = torch.stack([r[:, 1] for r in z])
        for a in range(4):
            for b in range(4):
                want[a, b, 0] += (i[a] * i[b] + q[a] * q[b]).sum()
                want[a, b, 1] += (q[a] * i[b] - i[a] * q[b]).sum()
    want = want.cpu().numpy()
    tail = [x[2 * (WIDE - 5000):].cpu().numpy().reshape(-1, 2) for x in wide]
    tail_heads = [x[2 * (WIDE - 5001):2 * (WIDE - 5000)].cpu().numpy().reshape(-1, 2) for x in wide]
    z = rows_of(WIDE - 5000, WIDE)
    assert int((z[0][:, 1] * z[3][:, 0] - z[0][:, 0] * z[3][:, 1]).sum()) == int(sr.cov_ref(tail, tail_heads, WTAPS)[0, 3, 1])
    assert np.array_equal(got, want), (got.tolist(), want.tolist())

    w = np.array([[[3000, -1000], [200, 900]], [[-500, 2500], [-1100, 30]]], np.int16)
    shift = 20                                                         # |acc| <= 9230 * 32768 = 2^28.2: a few outputs in a hundred clamp at +-127
    dst = torch.full((2 * WIDE + 128,), 0x7F, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.stap_combine(ptrs, WIDE, SC16, w, shift, SC08, dst.data_ptr() + 64, heads=hptrs)
    assert (dst[:64] == 0x7F).all() and (dst[64 + 2 * WIDE:] == 0x7F).all()
    for lo, hi in ((WIDE - 6000, WIDE), (2 ** 29 - 3000, 2 ** 29 + 3000), (0, 3000)):
        xs = [x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2) for x in wide]
        hs = heads_np if lo == 0 else [x[2 * (lo - 1):2 * lo].cpu().numpy().reshape(-1, 2) for x in wide]
        ref, _ = sr.combine_ref(xs, hs, w, shift, SC08)
        out = dst[64 + 2 * lo:64 + 2 * hi].cpu().numpy().view(np.int8).reshape(-1, 2)
        assert np.array_equal(out, ref), (lo, hi)
    count = 0
    for lo in range(0, WIDE, chunk):
        z = rows_of(lo, min(lo + chunk, WIDE))
        wk = w.reshape(-1, 2)
        acc_i = sum(int(wk[k, 0]) * z[k][:, 0] - int(wk[k, 1]) * z[k][:, 1] for k in range(4))
        acc_q = sum(int(wk[k, 0]) * z[k][:, 1] + int(wk[k, 1]) * z[k][:, 0] for k in range(4))
        for acc in (acc_i, acc_q):
            y = (acc + (1 << (shift - 1))) >> shift
            count += int(((y > 127) | (y < -127)).sum())
    assert clipped == count and count > 0
    del wide, dst
    torch.cuda.empty_cache()
