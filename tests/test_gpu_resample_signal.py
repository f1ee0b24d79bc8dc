"""What the resampler is for, on the MI355X, read by the project's own instruments: a tone that moves to the bin the ratio sends it to,
a tone beyond the new Nyquist rate that the designed taps take out, a clock offset of 20 ppm held against a double-precision sinusoid
with and without interpolation between the phases, and a 2.6 Msps render found by gpsiq_acquire at 2.048 Msps where its descriptors,
the ratio and the group delay put it.  Every case is first run through the numpy restatements on the CPU (tests/_resample_ref.py,
_mix_ref.py, _spectrum_ref.py, _acquire_ref.py): the bounds come from what the reference alone reads, less 3 dB; the device stream is
then held to the reference's bytes AND read by the device instrument.  scripts/resample_signal.py writes the same cases' figures to
profiles/resample_signal.txt.  Run with -m gpu."""
import math

import numpy as np
import pytest

import _acquire_ref as ar
import _mix_ref as mr
import _oracle
import _resample_ref as rr
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import MIX_TONE, SC16, WINDOW_RECT
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

ONE = 1 << 32
NFFT, NSEG, SKIP = 512, 4, 32                      # SKIP outputs: the taps' transient at the head of a span
L, SHIFT = 7, 14
FIVE_FOURTHS = 5 << 30                             # 5/4 input samples an output: the rate falls to 4/5


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def db(x):
    return 10.0 * math.log10(x)


def power(x):
    return float(np.mean(np.sum(np.asarray(x, np.float64) ** 2, axis=1)))


def tone_through(ctx, tone_step, taps):
    """a gpsiq_mix tone of amplitude 25 000 resampled by 5/4 on the device, both stages held to their restatements' bytes ->
    (input [n, 2], reference output [NFFT * NSEG, 2] behind the transient, the device tensor of the whole output)"""
    import torch
    nout = NFFT * NSEG + SKIP
    nin = ((nout * FIVE_FOURTHS) >> 32) + 1
    term = mr.Term(MIX_TONE, 100, step=tone_step)
    x, _ = mr.mix_ref(nin, 0, [term], 0, 32767, np.int16)
    want, wc, wn, _ = rr.resample_ref(x, None, taps, L, SHIFT, 1, FIVE_FOURTHS, 0, SC16)
    assert wn >= nout and wc == 0
    src = torch.zeros(4 * nin, dtype=torch.uint8, device="cuda")
    ctx.mix(nin, 0, [term.mixterm()], 0, 32767, SC16, src.data_ptr())
    dst = torch.zeros(4 * wn, dtype=torch.uint8, device="cuda")
    n, _, c, _ = ctx.resample(nin, SC16, src.data_ptr(), taps, L, SHIFT, 1, FIVE_FOURTHS, 0, SC16, dst.data_ptr())
    assert n == wn and c == 0 and np.array_equal(dst.cpu().numpy().view(np.int16).reshape(-1, 2), want)
    return x, want[SKIP:nout], dst


def test_a_tone_moves_to_the_bin_the_ratio_sends_it_to(ctx):
    """32 cycles in 512 input samples are 40 cycles in 512 output samples at 5/4.  Through the restatements bins 39..41 hold 0.9999966 of
    the power; the device must read the peak in bin 40 and at least half that share (the reference's value less 3 dB)."""
    taps = gpsiq.resample_design(FIVE_FOURTHS, 0.8, L, 16, SHIFT)
    _, ref_y, dst = tone_through(ctx, 32 << 50, taps)
    shift = sr.min_shift(SC16, NFFT, WINDOW_RECT, NSEG)
    ref = sr.spectrum_ref(ref_y, NFFT, NFFT, WINDOW_RECT, NSEG, shift)[0].astype(np.float64)
    ref_share = ref[39:42].sum() / ref.sum()
    assert int(ref.argmax()) == 40 and ref_share >= 0.999                                   # the reference alone
    got = ctx.spectrum(NFFT * NSEG, SC16, dst.data_ptr() + 4 * SKIP, NFFT, NFFT, WINDOW_RECT, NSEG, shift)[0].astype(np.float64)
    share = got[39:42].sum() / got.sum()
    print(f"tone in bin 32 by 5/4: peak bin {int(got.argmax())}, share of bins 39..41 {share:.7f} (restatements {ref_share:.7f})")
    assert int(got.argmax()) == 40 and share >= ref_share / 2.0


def test_a_tone_beyond_the_new_nyquist_rate_is_taken_out(ctx):
    """0.45 of the input rate lies beyond 0.4, half the output rate at 5/4: the designed taps (cutoff 0.8 of that) must not let it fold
    back.  Through the restatements the output holds -46.39 dB of the input's power; the bound is 3 dB above that.  This guards the
    design, not the device: the bytes are the reference's anyway."""
    taps = gpsiq.resample_design(FIVE_FOURTHS, 0.8, L, 16, SHIFT)
    x, ref_y, dst = tone_through(ctx, int(round(0.45 * 2 ** 59)), taps)
    ref_att = db(power(ref_y) / power(x))
    assert ref_att <= -40.0                                                                 # the reference alone
    got = dst.cpu().numpy().view(np.int16).reshape(-1, 2)[SKIP:SKIP + NFFT * NSEG]
    att = db(power(got) / power(x))
    print(f"tone at 0.45 fs by 5/4: output power {att:.2f} dB of the input's (restatements {ref_att:.2f})")
    assert att <= ref_att + 3.0


def test_interpolation_between_phases_lowers_the_error_of_a_clock_offset(ctx):
    """A tone at 0.2 cycles a sample, amplitude 20 000, rounded to int16 from double precision, resampled at 1 + 20e-6 -- the fraction
    crosses all 128 phases once in 50 000 samples -- through 32 designed taps, against the double-precision sinusoid at the exact
    positions delayed by (ntaps-1)/2.  Through the restatements the error power is -44.86 dB of the tone's with the nearest phase below
    and -70.09 dB interpolated.  Asserted: interpolation is the lower, and within 3 dB of the restatements' value."""
    import torch
    step, ntaps, f, amp, nin, skip = round(ONE * (1 + 20e-6)), 32, 0.2, 20000.0, 60000, 100
    taps = gpsiq.resample_design(step, 0.9, L, ntaps, SHIFT)
    m = np.arange(nin)
    x = np.rint(amp * np.stack([np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)], axis=1)).astype(np.int16)
    src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    err_ref, err_dev = [], []
    for interp in (0, 1):
        want, wc, wn, _ = rr.resample_ref(x, None, taps, L, SHIFT, interp, step, 0, SC16)
        t = (np.arange(wn) * step) / ONE - (ntaps - 1) / 2
        ideal = amp * np.stack([np.cos(2 * np.pi * f * t), np.sin(2 * np.pi * f * t)], axis=1)
        dst = torch.zeros(4 * wn, dtype=torch.uint8, device="cuda")
        n, _, c, _ = ctx.resample(nin, SC16, src.data_ptr(), taps, L, SHIFT, interp, step, 0, SC16, dst.data_ptr())
        got = dst.cpu().numpy().view(np.int16).reshape(-1, 2)
        assert n == wn and c == wc == 0 and np.array_equal(got, want)
        err_ref.append(db(power(want[skip:] - ideal[skip:]) / amp ** 2))
        err_dev.append(db(power(got[skip:] - ideal[skip:]) / amp ** 2))
    assert err_ref[1] < err_ref[0] - 10.0 and err_ref[1] <= -60.0                          # the reference alone
    print(f"20 ppm, tone at 0.2 fs: error {err_dev[0]:.2f} dB nearest phase, {err_dev[1]:.2f} dB interpolated (restatements {err_ref[0]:.2f}, {err_ref[1]:.2f})")
    assert err_dev[1] < err_dev[0] and err_dev[1] <= err_ref[1] + 3.0


def test_a_render_at_one_rate_is_acquired_at_another(ctx):
    """A noiseless block of three satellites rendered at 2.6 Msps, resampled to 2.048 Msps with the designed 128 x 16 taps, searched
    with gpsiq_acquire_steps at 2.048e6 (a millisecond is 2 048 samples): every satellite in the Doppler bin of its f_carr, at the shift
    where its code reaches chip 0 -- input sample s, seen at output (s + (ntaps-1)/2) / ratio -- within one sample."""
    import torch
    fs_in, fs_out, nsamp, ntaps = 2.6e6, 2.048e6, 16384, 16
    ms = 2048
    S = dict(ncoh=ms, hop=ms, nnoncoh=4, f0=-5000.0, df=500.0, ndopp=21, nshift=ms, guard=3)
    step = gpsiq.resample_step(fs_in, fs_out)
    ratio = step / ONE
    taps = gpsiq.resample_design(step, 0.8, L, ntaps, SHIFT)
    d = synth_blocks(1, 3, seed=2048, doppler_hz=4400.0, prn0=5)
    d["gain"][:] = 1.0
    prns = [int(p) for p in d["prn"][0]]
    x = ctx.generate_batch(d, nsamp, fs_in, SC16).reshape(-1, 2)
    want, wc, wn, _ = rr.resample_ref(x, None, taps, L, SHIFT, 1, step, 0, SC16)
    assert wn >= (S["nshift"] - 1) + (S["nnoncoh"] - 1) * S["hop"] + S["ncoh"] and wc == 0
    code_step, c0, ci = gpsiq.acquire_steps(fs_out, S["f0"], S["df"])
    period = 1023.0 / (1.023e6 / fs_out)                                                   # samples of a code period at the nominal chip rate

    def expected(ch):
        s_in = ((1023.0 - ch["code_phase"]) % 1023.0) / (ch["f_code"] / fs_in)
        return int(np.rint((ch["f_carr"] - S["f0"]) / S["df"])), ((s_in + (ntaps - 1) / 2) / ratio) % period

    def near(shift, exp):
        return min((shift - exp) % period, (exp - shift) % period) <= 1.0

    # the reference alone
    _, ref, _ = ar.acquire(_oracle.load_oracle(), want.ravel(), prns, code_step, c0, ci, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
    for k, prn in enumerate(prns):
        b, s, _ = ar.decide(ref[k], S["guard"])
        eb, es = expected(d[0, k])
        assert b == eb and near(s, es), (prn, b, s, eb, es)
    # the device
    src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    dst = torch.zeros(4 * wn, dtype=torch.uint8, device="cuda")
    n, _, c, _ = ctx.resample(nsamp, SC16, src.data_ptr(), taps, L, SHIFT, 1, step, 0, SC16, dst.data_ptr())
    assert n == wn and c == 0 and np.array_equal(dst.cpu().numpy().view(np.int16).reshape(-1, 2), want)
    _, got, _, _ = ctx.acquire(wn, SC16, dst.data_ptr(), prns, code_step, c0, ci, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
    for k, prn in enumerate(prns):
        b, s, r = gpsiq.acquire_decide(got[k], S["guard"])
        eb, es = expected(d[0, k])
        print(f"PRN {prn}: f_carr {float(d['f_carr'][0, k]):+.1f} Hz, bin {b} (expected {eb}), shift {s} (expected {es:.2f}), ratio {r:.1f}")
        assert b == eb and near(s, es) and (b, s) == tuple(ar.decide(ref[k], S["guard"])[:2])
