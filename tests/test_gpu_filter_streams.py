"""Stream order of gpsiq_filter on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side
stream while the producer of its input still waits there behind a filler, and the null stream is busy until after it returns -- so
a tap upload, a memset of the counter, a kernel or a copy-back queued on the wrong stream gives wrong bytes or a wrong count.  The
caller overwrites its taps as soon as the call has returned, and a second ordered call uses different taps.  And the one wide-offset
case: 6e8 int16 samples, 2.4e9 bytes, filled on the device.  Run with -m gpu."""
import numpy as np
import pytest

import _filter_ref as fr
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0x7F


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_filter_runs_behind_the_producer_on_its_stream(ctx, scratch, side, monkeypatch, kernel):
    import torch
    monkeypatch.setenv("GPSIQ_FILTER_KERNEL", kernel)
    rng = np.random.default_rng(5)
    nsamp, decim, phase, shift = 9001, 3, 1, 6
    x = fr.full_range(rng, nsamp, SC08)
    true = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    buf = torch.full((2 * nsamp,), GUARD, dtype=torch.uint8, device="cuda")
    nout = fr.span(nsamp, decim, phase)[0]
    dst = torch.zeros(2 * nout + 64, dtype=torch.uint8, device="cuda")
    for seed in (1, 2):                                                # the second call: different taps
        taps = np.random.default_rng(seed).integers(-500, 501, size=65).astype(np.int16)
        want, wc = fr.filter_ref(x, None, taps, shift, decim, phase, SC08)
        assert wc > 0
        mine = taps.copy()
        buf.fill_(GUARD)
        dst.fill_(GUARD)
        ctx.filter(nsamp, SC08, buf.data_ptr(), mine, shift, decim, phase, SC08, dst.data_ptr())       # an ordinary call on the wrong input
        wrong = dst.cpu().numpy()[:2 * nout].view(np.int8).reshape(-1, 2)
        assert not np.array_equal(wrong, want)
        dst.fill_(GUARD)
        torch.cuda.synchronize()

        def stage(s):
            out = ctx.filter(nsamp, SC08, buf.data_ptr(), mine, shift, decim, phase, SC08, dst.data_ptr(), stream=s)
            mine[:] = 0                                                # the caller's taps are the caller's again
            return out

        n, clipped, _ = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True), stage)
        got = dst.cpu().numpy()
        assert ctx.filter_last_plan()[0] == kernel
        assert n == nout and clipped == wc and np.array_equal(got[:2 * nout].view(np.int8).reshape(-1, 2), want) and (got[2 * nout:] == GUARD).all()


def test_a_span_past_two_to_the_31_bytes(ctx):
    """int16, 6e8 samples: byte offsets pass 2^31 inside the span (2^32 lies beyond it).  The reference filters windows only: the
    first outputs, those whose windows straddle byte 2^31, and the last"""
    import torch
    nsamp, decim, phase, shift = 600_000_000, 16, 5, 14
    taps = gpsiq.filter_design(10.4e6, 0.3e6, 65, 14)
    torch.manual_seed(31)
    x = torch.randint(-32768, 32768, (2 * nsamp,), dtype=torch.int16, device="cuda")
    nout = fr.span(nsamp, decim, phase)[0]
    dst = torch.full((4 * nout + 64,), GUARD, dtype=torch.uint8, device="cuda")
    n, clipped, ms = ctx.filter(nsamp, SC16, x.data_ptr(), taps, shift, decim, phase, SC16, dst.data_ptr())
    assert n == nout and ctx.filter_last_plan()[0] == "generic"
    edge = (1 << 31) // 4                                              # the sample at byte 2^31
    j_edge = (edge - phase) // decim
    outputs = list(range(0, 40)) + list(range(j_edge - 8, j_edge + 12)) + list(range(nout - 40, nout))
    x_at = lambda lo, hi: x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2)
    want = fr.filter_windows(x_at, nsamp, taps, shift, decim, phase, SC16, outputs)
    idx = torch.tensor(outputs, device="cuda")
    got = dst[:4 * nout].view(torch.int16).reshape(-1, 2)[idx].cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert (dst[4 * nout:].cpu().numpy() == GUARD).all() and clipped == 0
    # windows on both sides of the edge were compared
    assert phase + (j_edge - 8) * decim - 64 < edge < phase + (j_edge + 11) * decim
    del x, dst
    torch.cuda.empty_cache()
