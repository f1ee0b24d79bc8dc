"""What the mix stage is for, on the MI355X, read by the project's own instruments: a tone and a chirp in gpsiq_spectrum, a repeater's
second correlation peak in gpsiq_acquire, a swept jammer's cost in gpsiq_despread + gpsiq_cn0_estimate.  Every case is first run
through the numpy restatements on the CPU (tests/_mix_ref.py, _spectrum_ref.py, _acquire_ref.py, _despread_ref.py), so that the
reference alone is known to satisfy the property; the device stream is then held to the reference's bytes AND read by the device
instrument.  Run with -m gpu."""
import math

import numpy as np
import pytest

import _acquire_ref as ar
import _despread_ref as dr
import _mix_ref as mr
import _oracle
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import MIX_ROTATED, MIX_STREAM, MIX_TONE, SC16, WINDOW_RECT
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

FS = 2.6e6
NFFT = 512


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def mixed_on_the_device(ctx, nsamp, terms, shift, want):
    """a tone-only mix into a fresh int16 device buffer, held to the restatement's bytes -> the tensor"""
    import torch
    dst = torch.zeros(4 * nsamp, dtype=torch.uint8, device="cuda")
    ctx.mix(nsamp, 0, [t.mixterm() for t in terms], shift, 32767, SC16, dst.data_ptr())
    assert np.array_equal(dst.cpu().numpy().view(np.int16).reshape(-1, 2), want)
    return dst


@pytest.mark.parametrize("sign,peak", [(1, 37), (-1, 475)])
def test_a_tone_is_a_line_in_its_bin(ctx, sign, peak):
    """A tone at step +-37 * 2^50 -- 37 table entries a sample, 37 cycles in 512 samples -- peaks in bin 37 / 512 - 37 of a rectangular
    512-point spectrum and holds >= 99 % of the power there: the sign convention of the contract.  (The table's rounding, at most 0.5
    in 250, leaves about 4e-6 of the power elsewhere.)"""
    nseg = 4
    n = NFFT * nseg
    terms = [mr.Term(MIX_TONE, 100, step=sign * (37 << 50))]
    want, _ = mr.mix_ref(n, 0, terms, 0, 32767, np.int16)
    shift = sr.min_shift(SC16, NFFT, WINDOW_RECT, nseg)
    ref = sr.spectrum_ref(want, NFFT, NFFT, WINDOW_RECT, nseg, shift)[0].astype(np.float64)
    assert int(ref.argmax()) == peak and ref[peak] >= 0.99 * ref.sum()                     # the reference alone
    dst = mixed_on_the_device(ctx, n, terms, 0, want)
    got = ctx.spectrum(n, SC16, dst.data_ptr(), NFFT, NFFT, WINDOW_RECT, nseg, shift)[0].astype(np.float64)
    print(f"step {sign:+d} * 37 * 2^50: peak bin {int(got.argmax())}, share {got[peak] / got.sum():.7f}")
    assert int(got.argmax()) == peak and got[peak] >= 0.99 * got.sum()


def test_a_chirp_fills_the_band_it_sweeps(ctx):
    """gpsiq.mix_tone(fs, -fs/8, +fs/8, 8192 samples): a quarter of the band, bins -64 .. +64 of 512.  Over 64 segments (four sweeps)
    the restatement puts 99.99 % of the power inside the swept bins +- 8 (>= 95 % is asked of it); the device stream must hold >= 90 %.
    The bytes are equal anyway: this pins the helper and the sign."""
    period, nseg = 8192, 64
    n = NFFT * nseg
    step, rate, per = gpsiq.mix_tone(FS, -FS / 8, FS / 8, period / FS)
    assert per == period and step < 0 < rate
    terms = [mr.Term(MIX_TONE, 100, step=step, rate=rate, sweep=(per, 0))]
    want, _ = mr.mix_ref(n, 0, terms, 0, 32767, np.int16)
    shift = sr.min_shift(SC16, NFFT, WINDOW_RECT, nseg)
    k = np.arange(NFFT)
    inside = np.abs(np.where(k < NFFT // 2, k, k - NFFT)) <= NFFT // 8 + 8
    ref = sr.spectrum_ref(want, NFFT, NFFT, WINDOW_RECT, nseg, shift)[0].astype(np.float64)
    assert ref[inside].sum() >= 0.95 * ref.sum()                                           # the reference alone
    dst = mixed_on_the_device(ctx, n, terms, 0, want)
    got = ctx.spectrum(n, SC16, dst.data_ptr(), NFFT, NFFT, WINDOW_RECT, nseg, shift)[0].astype(np.float64)
    share = got[inside].sum() / got.sum()
    flat = got[inside][8:-8]
    print(f"chirp -fs/8 .. +fs/8: {share:.6f} of the power inside bins +-{NFFT // 8 + 8}; swept bins max / min {flat.max() / flat.min():.3f}")
    assert share >= 0.90


def test_a_repeater_is_a_second_peak(ctx):
    """A noiseless rendered block plus itself delayed by 700 samples and turned by four Doppler bins of tests/_acquire_ref.py's search
    (2 000 Hz, towards the middle of the grid): gpsiq_acquire finds the satellite at shift s0 in the direct bin and at s0 + 700 (mod
    the 2 600 samples of a code period) in the bin four further."""
    import torch
    S = ar.SEARCH
    nsamp, delay = 16384, 700
    assert 3 * S["hop"] + S["ncoh"] + S["nshift"] + delay <= nsamp
    d = synth_blocks(1, 1, seed=2600, doppler_hz=4400.0, prn0=5)
    prn, f_carr = int(d["prn"][0, 0]), float(d["f_carr"][0, 0])
    code_step, c0, ci = gpsiq.acquire_steps(FS, S["f0"], S["df"])
    bin_d = int(np.rint((f_carr - S["f0"]) / S["df"]))
    hops = -4 if f_carr > 0 else 4
    bin_r = bin_d + hops
    assert 0 <= bin_r < S["ndopp"]
    x = ctx.generate_batch(d, nsamp, FS, SC16).reshape(-1, 2)
    terms = [mr.Term(MIX_STREAM, 1 << 8, x), mr.Term(MIX_ROTATED, 1, x[:nsamp - delay], skip=delay, step=hops * ci)]
    want, wc = mr.mix_ref(nsamp, 0, terms, 8, 32767, np.int16)
    # the reference alone, at the two bins
    lo = min(bin_d, bin_r)
    _, power, _ = ar.acquire(_oracle.load_oracle(), want.ravel(), [prn], code_step, c0 + lo * ci, 4 * ci, 2, S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
    rows = {lo: power[0][0], lo + 4: power[0][1]}
    s0 = int(rows[bin_d].argmax())
    exp = ar.expected_cell(d[0, 0], FS)
    assert exp[0] == bin_d and min((s0 - exp[1]) % S["nshift"], (exp[1] - s0) % S["nshift"]) <= 1
    assert int(rows[bin_r].argmax()) == (s0 + delay) % S["nshift"]
    # the device
    src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    dst = torch.zeros_like(src)
    clipped, _ = ctx.mix(nsamp, 0, [terms[0].mixterm(src.data_ptr()), terms[1].mixterm(src.data_ptr())], 8, 32767, SC16, dst.data_ptr())
    assert np.array_equal(dst.cpu().numpy().view(np.int16).reshape(-1, 2), want) and clipped == wc == 0
    _, got, _, _ = ctx.acquire(nsamp, SC16, dst.data_ptr(), [prn], code_step, c0, ci, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
    best = gpsiq.acquire_decide(got[0], S["guard"])
    print(f"PRN {prn}: direct bin {bin_d} shift {int(got[0][bin_d].argmax())}, repeated bin {bin_r} shift {int(got[0][bin_r].argmax())}, decision {best}")
    assert best[0] in (bin_d, bin_r)
    assert int(got[0][bin_d].argmax()) == s0 and int(got[0][bin_r].argmax()) == (s0 + delay) % S["nshift"]
    # and they are peaks: each stands well above its own row away from it
    for b in (bin_d, bin_r):
        row = got[0][b]
        far = np.delete(row, [(int(row.argmax()) + k) % len(row) for k in range(-3, 4)])
        assert row.max() > 10.0 * far.max()


def test_a_swept_jammer_costs_what_its_density_predicts(ctx):
    """tests/_despread_ref.py's closed loop -- one channel at gain 2 and 45 dB-Hz, 64 blocks of 66 560 samples at 2.6 Msps, 1 664
    segments -- plus a chirp that sweeps the WHOLE sampled band every 1 021 samples (rate * period = 2^59) at amplitude 31 * 250: its
    density is J / fs with J = 7 750^2, N0 = 2 sigma^2 / fs, so the predicted loss is -10 log10(1 + J / (2 sigma^2)) = -5.935 dB.
    The difference of the two gpsiq_cn0_estimate readings must match it within 4 sqrt(s1^2 + s2^2) + the model allowance, s1 and s2 the
    estimates' own one_sigma_db (0.108 and 0.113 dB).  Model allowance: through the numpy restatements alone the same case reads
    44.895 -> 39.040 dB-Hz, -5.854 dB, 0.081 dB short of the prediction (a chirp is not white noise to a correlator); with 0.2 dB for
    rounding that is 0.281 dB, and the bound 0.906 dB.  (Other periods through the restatements: 257: 0.187, 4 099: 0.142, 16 411:
    0.361 dB short.)"""
    import torch
    from test_despread_ref import loop_reference
    L = dr.LOOP
    allowance = 0.081 + 0.2
    q, stream, sums, _ = loop_reference()
    nb, ns, seg = L["nblocks"], L["nsamp"], L["seg_len"]
    n = nb * ns
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    period, gain = 1021, 31
    tone = mr.Term(MIX_TONE, gain, step=-(1 << 58), rate=(1 << 59) // period, sweep=(period, 0))
    pred = -10.0 * math.log10(1.0 + (gain * 250.0) ** 2 / (2.0 * sigma ** 2))
    # the reference alone
    want, wc = mr.mix_ref(n, 0, [mr.Term(MIX_STREAM, 1, stream.reshape(-1, 2)), tone], 0, 32767, np.int16)
    jammed, _ = dr.despread(_oracle.load_oracle(), q, want.reshape(nb, -1), ns, seg)
    (r1, s1), (r2, s2) = dr.cn0_estimate(sums[:, 0], seg, L["fs"]), dr.cn0_estimate(jammed[:, 0], seg, L["fs"])
    assert abs((r2 - r1) - pred) <= 1.0 and abs((r2 - r1) - pred) <= allowance - 0.2 + 0.005
    # the device: render, measure, jam where the stream lies, measure again
    buf = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.set_noise(L["seed"], sigma, 0)
    try:
        ctx.set_descriptors(q)
        ctx.launch(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, stream=s)
        clean = ctx.despread(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, seg, stream=s)[0]
        clipped, _ = ctx.mix(n, 0, [gpsiq.MixTerm.stream(buf.data_ptr(), SC16, 1), tone.mixterm()], 0, 32767, SC16, buf.data_ptr(), stream=s)
        assert clipped == wc and np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), want)
        dirty = ctx.despread(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, seg, stream=s)[0]
    finally:
        ctx.noise_off()
    (g1, t1), (g2, t2) = gpsiq.cn0_estimate(clean[:, 0], seg, L["fs"]), gpsiq.cn0_estimate(dirty[:, 0], seg, L["fs"])
    bound = 4.0 * math.sqrt(t1 * t1 + t2 * t2) + allowance
    print(f"C/N0 {g1:.3f} -> {g2:.3f} dB-Hz: {g2 - g1:+.3f} dB, predicted {pred:+.3f}, off by {g2 - g1 - pred:+.3f} (bound {bound:.3f}); "
          f"one sigma {t1:.3f}, {t2:.3f}; the restatements read {r2 - r1:+.3f}")
    assert abs((g2 - g1) - pred) <= bound
