"""Stream order of gpsiq_resample on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side
stream while the producer of its input still waits there behind a filler, and the null stream is busy until after it returns -- so
a table upload, a memset of the counter, a kernel or a copy-back queued on the wrong stream gives wrong bytes or a wrong count.  The
caller overwrites its table as soon as the call has returned, and a second ordered call uses a different one.  And the one wide
case: int8 upsampled eight times into int16, more than 2^30 outputs, a destination past 2^32 bytes.  Run with -m gpu."""
import numpy as np
import pytest

import _resample_ref as rr
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ONE = 1 << 32
GUARD = 0x7F


@pytest.mark.parametrize("kernel", ["generic", "rows"])
def test_resample_runs_behind_the_producer_on_its_stream(ctx, scratch, side, monkeypatch, kernel):
    import torch
    monkeypatch.setenv("GPSIQ_RESAMPLE_KERNEL", kernel)
    rng = np.random.default_rng(5)
    nsamp, L, ntaps, shift, step, pos0 = 9001, 5, 16, 6, round(ONE * 2.6 / 2.048), ONE - 1
    x = rr.full_range(rng, nsamp, SC08)
    true = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    buf = torch.full((2 * nsamp,), GUARD, dtype=torch.uint8, device="cuda")
    nout, nxt = rr.span(nsamp, pos0, step)
    dst = torch.zeros(2 * nout + 64, dtype=torch.uint8, device="cuda")
    for seed in (1, 2):                                                # the second call: a different table
        taps = np.random.default_rng(seed).integers(-2000, 2001, size=((1 << L) + 1, ntaps)).astype(np.int16)
        want, wc, _, _ = rr.resample_ref(x, None, taps, L, shift, 1, step, pos0, SC08)
        assert wc > 0
        mine = taps.copy()
        buf.fill_(GUARD)
        dst.fill_(GUARD)
        ctx.resample(nsamp, SC08, buf.data_ptr(), mine, L, shift, 1, step, pos0, SC08, dst.data_ptr())      # an ordinary call on the wrong input
        wrong = dst.cpu().numpy()[:2 * nout].view(np.int8).reshape(-1, 2)
        assert not np.array_equal(wrong, want)
        dst.fill_(GUARD)
        torch.cuda.synchronize()

        def stage(s):
            out = ctx.resample(nsamp, SC08, buf.data_ptr(), mine, L, shift, 1, step, pos0, SC08, dst.data_ptr(), stream=s)
            mine[:] = 0                                                # the caller's table is the caller's again
            return out

        n, got_next, clipped, _ = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True), stage)
        got = dst.cpu().numpy()
        assert ctx.resample_last_plan()[0] == kernel
        assert (n, got_next) == (nout, nxt) and clipped == wc
        assert np.array_equal(got[:2 * nout].view(np.int8).reshape(-1, 2), want) and (got[2 * nout:] == GUARD).all()


def test_more_than_two_to_the_30_outputs_into_more_than_two_to_the_32_bytes(ctx, monkeypatch):
    """int8 in, int16 out, step 2^29: j passes 2^30 and the byte offset of an output 2^32.  The designed taps cannot clip an int8 stream
    into int16 (|y| <= 65535 * 128 / 2^14), so the count must be 0.  The reference resamples windows of j only: the first outputs, those
    around byte offsets 2^31 and 2^32 of the destination, and the last"""
    import torch
    monkeypatch.delenv("GPSIQ_RESAMPLE_KERNEL", raising=False)
    nsamp, L, ntaps, shift, step, pos0 = (1 << 27) + 1000, 7, 16, 14, 1 << 29, 3
    taps = gpsiq.resample_design(step, 0.8, L, ntaps, shift)
    torch.manual_seed(32)
    x = torch.randint(-128, 128, (2 * nsamp,), dtype=torch.int8, device="cuda")
    nout, nxt = rr.span(nsamp, pos0, step)
    assert nout > 1 << 30 and 4 * nout > 1 << 32
    dst = torch.full((4 * nout + 64,), GUARD, dtype=torch.uint8, device="cuda")
    n, got_next, clipped, ms = ctx.resample(nsamp, SC08, x.data_ptr(), taps, L, shift, 1, step, pos0, SC16, dst.data_ptr())
    assert (n, got_next) == (nout, nxt) and clipped == 0
    x_at = lambda lo, hi: x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2)
    out = dst[:4 * nout].view(torch.int16).reshape(-1, 2)
    for j_lo, j_hi in ((0, 600), ((1 << 29) - 300, (1 << 29) + 300), ((1 << 30) - 300, (1 << 30) + 300), (nout - 600, nout)):
        want, wc = rr.resample_window(x_at, nsamp, taps, L, shift, 1, step, pos0, SC16, j_lo, j_hi)
        got = out[j_lo:j_hi].cpu().numpy()
        assert wc == 0 and np.array_equal(got, want), (j_lo, np.argwhere(got != want)[:4])
        assert np.abs(want).max() > 0
    assert (dst[4 * nout:].cpu().numpy() == GUARD).all()
    del x, dst, out
    torch.cuda.empty_cache()
