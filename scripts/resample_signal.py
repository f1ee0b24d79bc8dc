"""profiles/resample_signal.txt: what the project's instruments read off streams gpsiq_resample has made -- measured values, written
down, not thresholds (the thresholds are in tests/test_gpu_resample_signal.py, which runs the same cases).
  1  a gpsiq_mix tone in bin 32 of 512, resampled by 5/4 (designed 128 x 16 taps): the peak bin of gpsiq_spectrum and the share of bins 39..41
  2  a tone at 0.45 of the input rate, resampled by 5/4, beyond the new Nyquist rate: the output's power against the input's
  3  an int16 tone at 0.2 cycles a sample resampled at 1 + 20e-6, against a double-precision sinusoid at the exact positions delayed by
     (ntaps-1)/2: the error power without and with interpolation between the phases, for 128 x 16 and 128 x 32 designed taps
  4  a noiseless 2.6 Msps render of three satellites resampled to 2.048 Msps and searched by gpsiq_acquire at 2.048e6: bin and shift
     found against the descriptor's
usage: timeout -k 10 300 python scripts/resample_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC16, WINDOW_RECT  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

ONE = 1 << 32
NFFT, NSEG, SKIP = 512, 4, 32
L, SHIFT = 7, 14
T = gpsiq.MixTerm


def power(x):
    return float(np.mean(np.sum(np.asarray(x, np.float64) ** 2, axis=1)))


def resampled(ctx, src, nin, taps, interp, step):
    """-> int16 [nout, 2] from the device tensor src, and the device tensor of the output"""
    nout = gpsiq.resample_span(nin, 0, step)[0]
    dst = torch.zeros(4 * nout, dtype=torch.uint8, device="cuda")
    n, _, clipped, _ = ctx.resample(nin, SC16, src.data_ptr(), taps, L, SHIFT, interp, step, 0, SC16, dst.data_ptr())
    assert n == nout and clipped == 0
    return dst.cpu().numpy().view(np.int16).reshape(-1, 2), dst


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    lines = [f"# python scripts/resample_signal.py: the instruments on streams made by gpsiq_resample, kernel id {gpsiq.kernels_id()}"]
    step = 5 << 30
    taps = gpsiq.resample_design(step, 0.8, L, 16, SHIFT)
    nout = NFFT * NSEG + SKIP
    nin = ((nout * step) >> 32) + 1
    shift = gpsiq.spectrum_min_shift(SC16, NFFT, WINDOW_RECT, NSEG)
    for name, tone in (("bin 32 of 512", 32 << 50), ("0.45 of the input rate", int(round(0.45 * 2 ** 59)))):
        src = torch.zeros(4 * nin, dtype=torch.uint8, device="cuda")
        ctx.mix(nin, 0, [T.tone(100, tone)], 0, 32767, SC16, src.data_ptr())
        x = src.cpu().numpy().view(np.int16).reshape(-1, 2)
        y, dst = resampled(ctx, src, nin, taps, 1, step)
        p = ctx.spectrum(NFFT * NSEG, SC16, dst.data_ptr() + 4 * SKIP, NFFT, NFFT, WINDOW_RECT, NSEG, shift)[0].astype(np.float64)
        lines.append(f"tone at {name}, by 5/4, 128 x 16 taps | peak bin {int(p.argmax())} | share of bins 39..41 {p[39:42].sum() / p.sum():.7f} | "
                     f"output power {10 * math.log10(power(y[SKIP:nout]) / power(x)):+.2f} dB of the input's")
    step, f, amp, nin, skip = gpsiq.resample_step(1.0, 1.0, -20000.0), 0.2, 20000.0, 60000, 100
    m = np.arange(nin)
    x = np.rint(amp * np.stack([np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)], axis=1)).astype(np.int16)
    src = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    for ntaps, bw in ((16, 0.8), (32, 0.9)):
        taps = gpsiq.resample_design(step, bw, L, ntaps, SHIFT)
        err = []
        for interp in (0, 1):
            y, _ = resampled(ctx, src, nin, taps, interp, step)
            t = (np.arange(len(y)) * step) / ONE - (ntaps - 1) / 2
            ideal = amp * np.stack([np.cos(2 * np.pi * f * t), np.sin(2 * np.pi * f * t)], axis=1)
            err.append(10 * math.log10(power(y[skip:] - ideal[skip:]) / amp ** 2))
        lines.append(f"tone at 0.2 fs, step 2^32 (1 + 20e-6) = {step}, 128 x {ntaps} taps, bandwidth {bw} | error power against the exact sinusoid: "
                     f"nearest phase {err[0]:+.2f} dB | interpolated {err[1]:+.2f} dB")
    fs_in, fs_out, nsamp, ntaps, ms = 2.6e6, 2.048e6, 16384, 16, 2048
    step = gpsiq.resample_step(fs_in, fs_out)
    taps = gpsiq.resample_design(step, 0.8, L, ntaps, SHIFT)
    d = synth_blocks(1, 3, seed=2048, doppler_hz=4400.0, prn0=5)
    d["gain"][:] = 1.0
    prns = [int(p) for p in d["prn"][0]]
    src = torch.from_numpy(ctx.generate_batch(d, nsamp, fs_in, SC16).view(np.uint8).ravel().copy()).cuda()
    y, dst = resampled(ctx, src, nsamp, taps, 1, step)
    code_step, c0, ci = gpsiq.acquire_steps(fs_out, -5000.0, 500.0)
    _, got, _, _ = ctx.acquire(len(y), SC16, dst.data_ptr(), prns, code_step, c0, ci, 21, ms, ms, 4, ms)
    for k, prn in enumerate(prns):
        ch = d[0, k]
        b, s, r = gpsiq.acquire_decide(got[k], 3)
        s_in = ((1023.0 - ch["code_phase"]) % 1023.0) / (ch["f_code"] / fs_in)
        exp = ((s_in + (ntaps - 1) / 2) / (step / ONE)) % (1023.0 / (1.023e6 / fs_out))
        lines.append(f"2.6 to 2.048 Msps, PRN {prn} at {float(ch['f_carr']):+.1f} Hz | bin {b} (nearest to f_carr: {int(np.rint((ch['f_carr'] + 5000.0) / 500.0))}) | "
                     f"shift {s} (descriptor, ratio and group delay: {exp:.2f}) | ratio {r:.1f}")
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
