"""The notch chain on the MI355X: spectrum -> gpsiq_notch_find -> gpsiq_notch_design -> gpsiq_cfilter -> spectrum, on an int16 stream of
8 192 samples built in numpy (tests/_cfilter_ref.py, notch_stream: seeded Gaussian noise, sigma 200 per component, plus a tone of
amplitude 8 000 on bin 37 of 256; the second case adds one on bin -90).  The three conditions -- the lines named are exactly those
put in, the filtered bytes are the restatement's, the output's spectrum holds no line -- are properties of the integer restatements
and tests/test_cfilter_ref.py establishes them there (seed 20261: the lines stand 51.3 dB over the floor, and after the notch the
largest cell stands 3.4 / 3.2 times over it against the ratio of 8).  The device must EQUAL the restatements, so there is no
tolerance of this file's own.  Both kernels.  Run with -m gpu."""
import numpy as np
import pytest

import _cfilter_ref as cr
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import SC16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def device_spectrum(ctx, t, nsamp):
    return ctx.spectrum(nsamp, SC16, t.data_ptr(), cr.NOTCH_NFFT, hop=cr.NOTCH_HOP, window=1)


def ref_spectrum(x):
    nseg, _ = sr.span(len(x), cr.NOTCH_NFFT, cr.NOTCH_HOP, 1)
    return sr.spectrum_ref(x, cr.NOTCH_NFFT, cr.NOTCH_HOP, 1, nseg, sr.min_shift(SC16, cr.NOTCH_NFFT, 1, nseg))


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("case", sorted(cr.NOTCH_CASES))
def test_the_lines_are_found_notched_and_gone(ctx, monkeypatch, case, kernel):
    import torch
    monkeypatch.setenv("GPSIQ_CFILTER_KERNEL", kernel)
    bins = cr.NOTCH_CASES[case]
    x = cr.notch_stream(bins)
    nsamp = len(x)
    src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    power = device_spectrum(ctx, src, nsamp)
    assert power.shape == (1, cr.NOTCH_NFFT) and np.array_equal(power, ref_spectrum(x))
    f, ex, n = gpsiq.notch_find(power[0], cr.NOTCH_FS, cr.NOTCH_RATIO, 8)
    assert n == len(bins) and sorted(np.rint(f / cr.bin_hz(1)).astype(int)) == sorted(bins)
    taps = gpsiq.notch_design(cr.NOTCH_FS, f, cr.NOTCH_WIDTH_BINS * cr.bin_hz(1), cr.NOTCH_NTAPS, cr.NOTCH_SHIFT)
    dst = torch.zeros(4 * nsamp, dtype=torch.uint8, device="cuda")
    nout, clipped, _ = ctx.cfilter(nsamp, SC16, src.data_ptr(), taps, cr.NOTCH_SHIFT, 1, 0, SC16, dst.data_ptr())
    assert ctx.cfilter_last_plan()[0] == {"generic": "generic", "mfma": "mfma16"}[kernel]
    want, wc = cr.cfilter_ref(x, None, taps, cr.NOTCH_SHIFT, 1, 0, SC16)
    assert nout == nsamp and clipped == wc and np.array_equal(dst.cpu().numpy().view(np.int16).reshape(-1, 2), want)
    after = device_spectrum(ctx, dst, nsamp)
    assert np.array_equal(after, ref_spectrum(want))
    assert gpsiq.notch_find(after[0], cr.NOTCH_FS, cr.NOTCH_RATIO, 8)[2] == 0
