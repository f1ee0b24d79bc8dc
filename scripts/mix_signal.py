"""profiles/mix_signal.txt: what the project's instruments read off streams gpsiq_mix has built -- measured values, written down, not
thresholds (the thresholds are in tests/test_gpu_mix_signal.py, which runs the same cases).
  1  a tone at step +-37 * 2^50 into int16, 512-point rectangular spectrum: the peak bin and its share of the power
  2  a chirp of gpsiq_mix_tone(fs, -fs/8, +fs/8, 8192 samples): the share of the power inside the swept bins +- 8, and the flatness there
  3  a repeater: a noiseless block plus itself delayed by 700 samples and turned by 2 kHz, searched by gpsiq_acquire: the two peaks
  4  a swept jammer over the whole band on a 45 dB-Hz channel (64 blocks of 66 560 samples): gpsiq_cn0_estimate before and after,
     against -10 log10(1 + J / (2 sigma^2)), for four sweep periods and three jammer levels
usage: timeout -k 10 300 python scripts/mix_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
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

FS, NFFT = 2.6e6, 512
T = gpsiq.MixTerm


def tone_spectrum(ctx, terms, nseg):
    n = NFFT * nseg
    dst = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    ctx.mix(n, 0, terms, 0, 32767, SC16, dst.data_ptr())
    shift = gpsiq.spectrum_min_shift(SC16, NFFT, WINDOW_RECT, nseg)
    return ctx.spectrum(n, SC16, dst.data_ptr(), NFFT, NFFT, WINDOW_RECT, nseg, shift)[0].astype(np.float64)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mix_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# python scripts/mix_signal.py: the instruments on streams built by gpsiq_mix, {FS / 1e6} Msps, kernel id {gpsiq.kernels_id()}"]
    for sign in (1, -1):
        p = tone_spectrum(ctx, [T.tone(100, sign * (37 << 50))], 4)
        k = int(p.argmax())
        lines.append(f"tone, step {sign:+d} * 37 * 2^50 | peak bin {k} | share of the power in it {p[k] / p.sum():.7f} | the rest {1.0 - p[k] / p.sum():.2e}")
    step, rate, period = gpsiq.mix_tone(FS, -FS / 8, FS / 8, 8192 / FS)
    p = tone_spectrum(ctx, [T.tone(100, step, rate=rate, sweep=(period, 0))], 64)
    k = np.arange(NFFT)
    k = np.where(k < NFFT // 2, k, k - NFFT)
    inside, flat = np.abs(k) <= NFFT // 8 + 8, np.abs(k) <= NFFT // 8 - 8
    lines.append(f"chirp -fs/8 .. +fs/8 every {period} samples, 64 segments | inside bins +-{NFFT // 8 + 8}: {p[inside].sum() / p.sum():.6f} | "
                 f"bins +-{NFFT // 8 - 8}: max / min {p[flat].max() / p[flat].min():.3f}")
    # the repeater, with the search of the acquisition tests
    ncoh, hop, nn, f0, df, ndopp, nshift, nsamp, delay = 2560, 2600, 4, -5000.0, 500.0, 21, 2600, 16384, 700
    d = synth_blocks(1, 1, seed=2600, doppler_hz=4400.0, prn0=5)
    prn, f_carr = int(d["prn"][0, 0]), float(d["f_carr"][0, 0])
    code_step, c0, ci = gpsiq.acquire_steps(FS, f0, df)
    hops = -4 if f_carr > 0 else 4
    src = torch.from_numpy(ctx.generate_batch(d, nsamp, FS, SC16).view(np.uint8).ravel().copy()).cuda()
    dst = torch.zeros_like(src)
    ctx.mix(nsamp, 0, [T.stream(src.data_ptr(), SC16, 1 << 8), T.rotated(src.data_ptr(), SC16, 1, hops * ci, skip=delay)], 8, 32767, SC16, dst.data_ptr())
    _, power, _, _ = ctx.acquire(nsamp, SC16, dst.data_ptr(), [prn], code_step, c0, ci, ndopp, nshift, ncoh, nn, hop)
    bin_d = int(np.rint((f_carr - f0) / df))
    for name, b in (("direct", bin_d), ("repeated", bin_d + hops)):
        row = power[0][b]
        far = np.delete(row, [(int(row.argmax()) + j) % len(row) for j in range(-3, 4)])
        lines.append(f"repeater, PRN {prn} at {f_carr:+.1f} Hz, delay {delay} samples, {hops * df:+.0f} Hz | {name} | bin {b} | shift {int(row.argmax())} | "
                     f"peak over the rest of its row {row.max() / far.max():.1f}")
    # the swept jammer
    nb, ns, seg, cn0, g = 64, 66560, 2560, 45.0, 2.0
    dd = synth_blocks(nb, 2, seed=45)
    dd["prn"][:, 0], dd["prn"][:, 1] = 7, 19
    dd["gain"][:, 0], dd["gain"][:, 1] = g, 0.0
    ctx.set_descriptors(gpsiq.quantize_blocks(dd, FS, ns)[0])
    sigma = gpsiq.noise_sigma_for_cn0(cn0, g, FS)
    buf = torch.empty(4 * nb * ns, dtype=torch.uint8, device="cuda")
    for period, gain in ((1021, 31), (257, 31), (4099, 31), (16411, 31), (1021, 13), (1021, 62)):
        ctx.set_noise(0xC0DE45, sigma, 0)
        ctx.launch(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, stream=s)
        clean = ctx.despread(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, seg, stream=s)[0]
        tone = T.tone(gain, -(1 << 58), rate=(1 << 59) // period, sweep=(period, 0))
        clipped, _ = ctx.mix(nb * ns, 0, [T.stream(buf.data_ptr(), SC16, 1), tone], 0, 32767, SC16, buf.data_ptr(), stream=s)
        dirty = ctx.despread(0, nb, ns, SC16, buf.data_ptr(), 4 * ns, seg, stream=s)[0]
        (a, sa), (b, sb) = gpsiq.cn0_estimate(clean[:, 0], seg, FS), gpsiq.cn0_estimate(dirty[:, 0], seg, FS)
        pred = -10.0 * math.log10(1.0 + (gain * 250.0) ** 2 / (2.0 * sigma ** 2))
        lines.append(f"swept jammer, whole band every {period} samples, amplitude {gain * 250}, J/S {20 * math.log10(gain * 250 / (250 * g)):.1f} dB | "
                     f"C/N0 {a:.3f} -> {b:.3f} dB-Hz | {b - a:+.3f} dB | predicted {pred:+.3f} | off by {b - a - pred:+.3f} | one sigma {sa:.3f}, {sb:.3f} | clipped {clipped}")
    ctx.noise_off()
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
