"""Stream order and wide offsets of gpsiq_stap_beams on the MI355X (include/gpsiq_rows.h, "Space-time array", "Several beams from one
pass").  Stream order as tests/test_gpu_stap_streams.py has it for the combiner (the fillers, the side stream and the two conditions
of tests/test_gpu_stage_streams.py are used as they are): the buffer the call reads -- streams and heads -- holds 0x7f until a
producer queued on a side stream behind a long filler puts the true input there; the call is made on that stream at once and must
return the restatement's answer for the true input.  Before each ordered call the same context makes an ordinary call on the 0x7f
bytes, so that its counters hold the answer to the wrong input.  Wide offsets: one int8 stream of 2^30 + 5000 samples, two taps, two
beams to int8, so that the byte offsets into the source and into both destinations pass 2^31.  Run with -m gpu."""
import numpy as np
import pytest

import _stap_beams_ref as br
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import copy_producer, guarded, ordered, scratch, side  # noqa: F401  (scratch and side are fixtures)
from test_gpu_stap_streams import staged_elements, NELEM, NSAMP, NTAPS

pytestmark = pytest.mark.gpu

NBEAMS = 3


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("in_size,out_size", [(SC08, SC16), (SC16, SC08)], ids=["8to16", "16to8"])
def test_the_beams_wait_for_their_producer(ctx, scratch, side, monkeypatch, kernel, in_size, out_size):  # noqa: F811
    import torch
    monkeypatch.setenv("GPSIQ_STAP_BEAMS_KERNEL", kernel)
    xs, heads, staged, at, hat = staged_elements(in_size)
    buf = guarded(staged)
    ptrs, hptrs = [buf.data_ptr() + a for a in at], [buf.data_ptr() + a for a in hat]
    w = np.random.default_rng(8).integers(-700, 701, size=(NBEAMS, NELEM, NTAPS, 2)).astype(np.int16)
    shift = 3 if in_size == SC08 else 19                               # some elements clamp, most do not
    want, wc = br.beams_ref(xs, heads, w, shift, out_size)
    assert all(0 < c < want[0].size // 2 for c in wc)
    olen = 2 * NSAMP * out_size
    step = -(-olen // 16) * 16
    dst = torch.zeros(NBEAMS * step, dtype=torch.uint8, device="cuda")
    dptrs = [dst.data_ptr() + b * step for b in range(NBEAMS)]
    wrong = ctx.stap_beams(ptrs, NSAMP, in_size, w, shift, out_size, dptrs, heads=hptrs)[0]
    assert all(a != b for a, b in zip(wrong, wc))                      # the counters hold the answer to the wrong input
    clipped, _ = ordered(scratch, side, copy_producer(buf, staged),
                         lambda s: ctx.stap_beams(ptrs, NSAMP, in_size, w, shift, out_size, dptrs, heads=hptrs, stream=s))
    assert ctx.stap_beams_last_plan()[0] == kernel
    got = dst.cpu().numpy()
    for b in range(NBEAMS):
        assert np.array_equal(got[b * step:b * step + olen].view(np.int8 if out_size == 1 else np.int16).reshape(-1, 2), want[b]), b
    assert np.array_equal(clipped, wc)


# ---- wide offsets ---------------------------------------------------------------------------------------------------------------------
WIDE = 2 ** 30 + 5000
TILE = 1 << 20
NEED = 3 * 2 * WIDE + (3 << 30)                                        # the stream, two outputs, and room to work in


def test_one_call_past_2_gib_of_the_source_and_of_both_destinations(ctx, monkeypatch):
    """Tile k of 2^20 samples is a fixed random tile plus k + 5 (k >> 8) in both components, wrapping in int8: tiles 256 apart differ
    too.  The bytes of both beams at the start (where the head is read), either side of byte offset 2^31 and at the very end against
    the restatement, and the counts over the whole span against torch's int64 arithmetic on the device (nothing of the library), that
    arithmetic itself held to the restatement on the last window.  Both kernels, on the same stream and the same expectations."""
    import torch
    free, total = torch.cuda.mem_get_info()
    assert free >= NEED, "the wide-offset test needs %.1f GiB of free device memory, %.1f of %.1f GiB are free" % (NEED / 2 ** 30, free / 2 ** 30, total / 2 ** 30)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2032)
    tile = torch.randint(-128, 128, (2 * TILE,), dtype=torch.int8, device="cuda", generator=gen)
    wide = torch.empty(2 * WIDE, dtype=torch.int8, device="cuda")
    for k in range(-(-WIDE // TILE)):
        lo, hi = 2 * k * TILE, min(2 * (k + 1) * TILE, 2 * WIDE)
        step = (k + 5 * (k >> 8)) & 255
        wide[lo:hi] = tile[:hi - lo] + (step - 256 if step > 127 else step)
    head_np = np.array([[-77, 101]], np.int8)
    head = torch.from_numpy(head_np.ravel().copy()).cuda()
    w = np.array([[[[9000, -3000], [700, 2900]]], [[[-1500, 7000], [-3300, 90]]]], np.int16)      # [2 beams][1 element][2 taps]
    shift = 13                                                         # |acc| <= 15600 * 128 = 2^21: a few outputs in a hundred clamp at +-127

    def window(lo, hi):
        xs = [wide[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2)]
        hs = [head_np] if lo == 0 else [wide[2 * (lo - 1):2 * lo].cpu().numpy().reshape(-1, 2)]
        return br.beams_ref(xs, hs, w, shift, SC08)

    windows = [(lo, hi, window(lo, hi)) for lo, hi in ((WIDE - 6000, WIDE), (2 ** 30 - 3000, 2 ** 30 + 3000), (0, 3000))]
    clipped = {}
    for kernel in ("generic", "mfma"):
        monkeypatch.setenv("GPSIQ_STAP_BEAMS_KERNEL", kernel)
        dsts = [torch.full((2 * WIDE + 128,), 0x7F, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        clipped[kernel], _ = ctx.stap_beams([wide.data_ptr()], WIDE, SC08, w, shift, SC08, [d.data_ptr() + 64 for d in dsts], heads=[head.data_ptr()])
        assert ctx.stap_beams_last_plan()[0] == kernel
        for d in dsts:
            assert (d[:64] == 0x7F).all() and (d[64 + 2 * WIDE:] == 0x7F).all()
        for lo, hi, (ref, _) in windows:
            for b in range(2):
                assert np.array_equal(dsts[b][64 + 2 * lo:64 + 2 * hi].cpu().numpy().view(np.int8).reshape(-1, 2), ref[b]), (kernel, b, lo, hi)
        del dsts

    def counts(lo, hi):
        now = wide[2 * lo:2 * hi].view(-1, 2).to(torch.int64)
        first = head.view(1, 2).to(torch.int64) if lo == 0 else wide[2 * (lo - 1):2 * lo].view(1, 2).to(torch.int64)
        z = [now, torch.cat([first, now[:-1]])]
        out = []
        for b in range(2):
            acc_i = sum(int(w[b, 0, t, 0]) * z[t][:, 0] - int(w[b, 0, t, 1]) * z[t][:, 1] for t in range(2))
            acc_q = sum(int(w[b, 0, t, 0]) * z[t][:, 1] + int(w[b, 0, t, 1]) * z[t][:, 0] for t in range(2))
            n = 0
            for acc in (acc_i, acc_q):
                y = (acc + (1 << (shift - 1))) >> shift
                n += int(((y > 127) | (y < -127)).sum())
            out.append(n)
        return np.array(out, dtype=np.uint64)

    assert np.array_equal(counts(WIDE - 6000, WIDE), windows[0][2][1])
    total_count, chunk = np.zeros(2, np.uint64), 1 << 25
    for lo in range(0, WIDE, chunk):
        total_count += counts(lo, min(lo + chunk, WIDE))
    assert np.array_equal(clipped["generic"], total_count) and np.array_equal(clipped["mfma"], total_count) and (total_count > 0).all()
    del wide
    torch.cuda.empty_cache()
