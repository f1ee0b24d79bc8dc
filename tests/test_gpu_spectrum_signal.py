"""gpsiq_filter's frequency response measured on a device stream by gpsiq_spectrum, on the MI355X: a seeded Gaussian int16 stream is
filtered on the device with gpsiq_filter_design(10.4e6, 1.2e6, 65, 14) at decim 1 into int16, and spectrum(out) / spectrum(in) is
compared per bin with |H(f)|^2 computed from those very taps.  Run with -m gpu."""
import math

import numpy as np
import pytest

import gpsiq
from gpsiq.abi import SC16, WINDOW_HANN

pytestmark = pytest.mark.gpu

FS, FC, NTAPS, TAP_SHIFT = 10.4e6, 1.2e6, 65, 14
NFFT, M, SIGMA = 512, 2048, 3000.0


def test_filter_response_on_a_device_stream():
    """Passband (|H|^2 >= 0.5): per bin within 6 / sqrt(M) relative, M = 2048 averaged segments -- six standard deviations of an averaged
    periodogram cell.  Stopband: the mean from 2 fc up at least 40 dB below the passband mean; the design's own bound is 0.002 in
    amplitude (-54 dB, tests/test_filter_ref.py), the 14 dB of margin are for Hann leakage and the int16 rounding.
    Measured on the MI355X: 111 passband bins, the worst 1.9 % off; the stopband mean 59.6 dB down.  The test prints both."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    ctx = gpsiq.Context(0)
    try:
        rng = np.random.default_rng(1207)
        nsamp = NFFT * M
        x = np.clip(np.rint(rng.normal(0.0, SIGMA, size=(nsamp, 2))), -32767, 32767).astype(np.int16)
        src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
        dst = torch.zeros(4 * nsamp, dtype=torch.uint8, device="cuda")
        taps = gpsiq.filter_design(FS, FC, NTAPS, TAP_SHIFT)
        nout, clipped, _ = ctx.filter(nsamp, SC16, src.data_ptr(), taps, TAP_SHIFT, 1, 0, SC16, dst.data_ptr())
        assert nout == nsamp and clipped == 0
        shift = gpsiq.spectrum_min_shift(SC16, NFFT, WINDOW_HANN, M)
        p_in = ctx.spectrum(nsamp, SC16, src.data_ptr(), NFFT, NFFT, WINDOW_HANN, M, shift)[0].astype(np.float64)
        p_out = ctx.spectrum(nsamp, SC16, dst.data_ptr(), NFFT, NFFT, WINDOW_HANN, M, shift)[0].astype(np.float64)
    finally:
        ctx.close()
    k = np.arange(NFFT)
    f = np.where(k < NFFT // 2, k, k - NFFT) * FS / NFFT
    h = (taps.astype(np.float64)[None, :] * np.exp(-2j * np.pi * f[:, None] * np.arange(NTAPS)[None, :] / FS)).sum(axis=1) / 2.0 ** TAP_SHIFT
    h2 = np.abs(h) ** 2
    ratio = p_out / p_in
    passband = h2 >= 0.5
    worst = float(np.abs(ratio[passband] / h2[passband] - 1.0).max())
    stop = np.abs(f) >= 2.0 * FC
    stop_db = 10.0 * math.log10(float(ratio[stop].mean()) / float(ratio[passband].mean()))
    density = float(p_in.mean()) * gpsiq.spectrum_scale(NFFT, WINDOW_HANN, M, shift, FS)
    print(f"passband bins {int(passband.sum())}: worst |ratio / |H|^2 - 1| = {worst:.4f} (bound {6 / math.sqrt(M):.4f}); "
          f"stopband bins {int(stop.sum())}: mean {stop_db:.1f} dB below the passband mean (bound -40); "
          f"input density / (2 sigma^2 / fs) = {density / (2 * SIGMA ** 2 / FS):.4f}")
    assert passband.sum() > 100 and stop.sum() > 200
    assert worst <= 6.0 / math.sqrt(M)
    assert stop_db <= -40.0
