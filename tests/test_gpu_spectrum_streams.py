"""Stream order of gpsiq_spectrum on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side
stream while the producer of its span still waits there behind a filler, and the null stream is busy until after it returns -- so a
table or matrix upload, the zeroing of the result, a kernel or the copy-back queued on the wrong stream gives wrong bytes.  The
ordinary call before it uses the other window, so the ordered call is the first of its (nfft, window) on the context and queues
its table matrix itself.  And the wide-offset case: 6e8 int16 samples, 2.4e9 bytes, filled on the device, read as int16 by the generic
kernel and as 1.2e9 int8 samples by the matrix kernel.  Run with -m gpu."""
import numpy as np
import pytest

import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16, WINDOW_HANN, WINDOW_RECT
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0x7F


@pytest.mark.parametrize("kernel,nfft", [("generic", 128), ("mfma", 256)])
def test_spectrum_runs_behind_the_producer_on_its_stream(ctx, scratch, side, monkeypatch, kernel, nfft):
    import torch
    monkeypatch.setenv("GPSIQ_SPECTRUM_KERNEL", kernel)
    rng = np.random.default_rng(6)
    hop, navg, count = nfft // 2, 7, 45
    nsamp = (count - 1) * hop + nfft + 3
    x = sr.full_range(rng, nsamp, SC08)
    shift = sr.min_shift(SC08, nfft, WINDOW_HANN, navg)
    want = sr.spectrum_ref(x, nfft, hop, WINDOW_HANN, navg, shift)
    true = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    buf = torch.full((2 * nsamp,), GUARD, dtype=torch.uint8, device="cuda")
    wrong = ctx.spectrum(nsamp, SC08, buf.data_ptr(), nfft, hop, WINDOW_RECT, navg, shift)           # an ordinary call on the wrong input
    assert wrong.shape == want.shape and not np.array_equal(wrong, want)
    torch.cuda.synchronize()
    got = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True),
                  lambda s: ctx.spectrum(nsamp, SC08, buf.data_ptr(), nfft, hop, WINDOW_HANN, navg, shift, stream=s))
    assert ctx.spectrum_last_plan()[0] == kernel
    assert np.array_equal(got, want)
    # and once more, ordered again, now with everything cached: the zeroing and the copy-back alone
    buf.fill_(GUARD)
    torch.cuda.synchronize()
    got = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True),
                  lambda s: ctx.spectrum(nsamp, SC08, buf.data_ptr(), nfft, hop, WINDOW_HANN, navg, shift, stream=s))
    assert np.array_equal(got, want)


def test_a_span_past_two_to_the_31_bytes(ctx, monkeypatch):
    """Byte offsets pass 2^31 inside the span (2^32 lies beyond it).  The restatement sees three groups only: the first, the one whose
    samples straddle byte 2^31, and the last."""
    import torch
    monkeypatch.delenv("GPSIQ_SPECTRUM_KERNEL", raising=False)
    n16 = 600_000_000
    torch.manual_seed(32)
    x = torch.randint(-32768, 32768, (2 * n16,), dtype=torch.int16, device="cuda")
    nfft, hop, navg = 64, 64, 1000
    for ss, nsamp, kernel in ((SC16, n16, "generic"), (SC08, 2 * n16, "mfma")):
        monkeypatch.setenv("GPSIQ_SPECTRUM_KERNEL", kernel)
        shift = sr.min_shift(ss, nfft, WINDOW_HANN, navg)
        got = ctx.spectrum(nsamp, ss, x.data_ptr(), nfft, hop, WINDOW_HANN, navg, shift)
        nseg, ngroups = sr.span(nsamp, nfft, hop, navg)
        assert got.shape == (ngroups, nfft) and ctx.spectrum_last_plan()[0] == kernel
        per_sample = 2 * ss                                            # bytes
        edge = (1 << 31) // per_sample                                 # the sample at byte 2^31
        g_edge = edge // (navg * hop)
        assert g_edge * navg * hop < edge < (g_edge + 1) * navg * hop and g_edge < ngroups - 1
        raw = x.view(torch.int8) if ss == SC08 else x
        for g in (0, g_edge, ngroups - 1):
            lo = g * navg * hop
            part = raw[2 * lo:2 * (lo + navg * hop)].cpu().numpy().reshape(-1, 2)
            assert np.array_equal(sr.spectrum_ref(part, nfft, hop, WINDOW_HANN, navg, shift)[0], got[g]), (ss, g)
    del x
    torch.cuda.empty_cache()
