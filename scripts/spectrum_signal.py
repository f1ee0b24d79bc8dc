"""profiles/spectrum_signal.txt: what gpsiq_spectrum reads off the library's own streams -- measured values, written down, not thresholds.
  1  one noiseless C/A channel at 10.4 Msps: the main lobe against the first nulls (+-1.023 MHz) and the first side lobes (+-1.5345 MHz)
  2  the same channel rendered directly at 2.6 Msps against rendered at 10.4 Msps, filtered (gpsiq_filter_design(10.4e6, 1.2e6, 65, 14))
     and decimated by 4: the aliasing DESIGN.md 8g speaks of, as density ratios per band
  3  the noise stage through a gain-0 channel: the mean density against 2 sigma^2 / fs and its spread over the bins
  4  a levelled qmax 1 stream against its qmax 127 twin (one channel at 45 dB-Hz): density in units of the output's own mean square
  5  the table-rounding floor: a full-scale tone built from the table itself, the other bins against the tone's
Hann window, half overlap, every segment in one group, min_shift, unless a row says otherwise.
usage: timeout -k 10 300 python scripts/spectrum_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16, WINDOW_HANN, WINDOW_RECT  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

NB = 2
SEED = 0x5BEC


def freqs(nfft, fs):
    k = np.arange(nfft)
    return np.where(k < nfft // 2, k, k - nfft) * fs / nfft


def render(ctx, d, fs, ss):
    """NB blocks of 0.1 s back to back on the device -> (tensor, samples)"""
    nsamp = int(round(fs / 10))
    ctx.set_descriptors(gpsiq.quantize_blocks(d, fs, nsamp)[0])
    buf = torch.empty(NB * 2 * nsamp * ss, dtype=torch.uint8, device="cuda")
    ctx.launch(0, NB, nsamp, ss, buf.data_ptr(), 2 * nsamp * ss, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return buf, NB * nsamp


def density(ctx, buf, nsamp, ss, nfft, fs, window=WINDOW_HANN):
    hop = nfft // 2
    navg = gpsiq.spectrum_span(nsamp, nfft, hop, 1)[0]
    shift = gpsiq.spectrum_min_shift(ss, nfft, window, navg)
    p = ctx.spectrum(nsamp, ss, buf.data_ptr(), nfft, hop, window, navg, shift)[0].astype(np.float64)
    return p * gpsiq.spectrum_scale(nfft, window, navg, shift, fs), navg


def db(x):
    return 10.0 * math.log10(x)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    lines = [f"# python scripts/spectrum_signal.py: gpsiq_spectrum on the library's own streams, {NB} blocks of 0.1 s; kernel id {gpsiq.kernels_id()}"]
    d = synth_blocks(NB, 1, seed=88)
    d["prn"][:, 0] = 7
    d["gain"][:, 0] = 1.0

    # 1: the sinc^2 of a C/A channel
    fs = 10.4e6
    buf, n = render(ctx, d, fs, SC16)
    dens, navg = density(ctx, buf, n, SC16, 512, fs)
    f = freqs(512, fs)
    band = lambda lo, hi: dens[(np.abs(f) >= lo) & (np.abs(f) < hi)]
    peak = float(band(0.0, 100e3).mean())
    lines.append(f"1 | C/A channel, gain 1, int16, 10.4 Msps, nfft 512 ({navg} segments) | density |f| < 100 kHz {peak:.4e} per Hz | total power {dens.sum() * fs / 512:.1f} (250^2 = 62500) | "
                 f"first nulls (|f| within 20 kHz of 1.023 MHz) {db(float(band(1.003e6, 1.043e6).mean()) / peak):+.1f} dB | "
                 f"first side lobes (|f| within 100 kHz of 1.5345 MHz) {db(float(band(1.4345e6, 1.6345e6).mean()) / peak):+.1f} dB (sinc^2: -13.3 at the top) | "
                 f"second nulls (2.046 MHz) {db(float(band(2.026e6, 2.066e6).mean()) / peak):+.1f} dB")

    # 2: direct 2.6 Msps against filtered and decimated
    taps = gpsiq.filter_design(10.4e6, 1.2e6, 65, 14)
    dst = torch.zeros(4 * (n // 4), dtype=torch.uint8, device="cuda")
    nout, clipped, _ = ctx.filter(n, SC16, buf.data_ptr(), taps, 14, 4, 0, SC16, dst.data_ptr())
    filt, _ = density(ctx, dst, nout, SC16, 128, 2.6e6)
    direct_buf, n26 = render(ctx, d, 2.6e6, SC16)
    direct, navg = density(ctx, direct_buf, n26, SC16, 128, 2.6e6)
    f = freqs(128, 2.6e6)
    cols = []
    for lo, hi in ((0.0, 0.5e6), (0.5e6, 1.0e6), (1.0e6, 1.3e6)):
        m = (np.abs(f) >= lo) & (np.abs(f) < hi)
        cols.append(f"{lo / 1e6:.1f}-{hi / 1e6:.1f} MHz direct / filtered {db(float(direct[m].mean()) / float(filt[m].mean())):+.2f} dB")
    lines.append(f"2 | the same channel at 2.6 Msps, nfft 128 ({navg} segments): rendered directly against rendered at 10.4 Msps, 65 taps at 1.2 MHz, decimated by 4 "
                 f"({clipped} clipped) | " + " | ".join(cols) + f" | total power direct {direct.sum() * 2.6e6 / 128:.1f}, filtered {filt.sum() * 2.6e6 / 128:.1f}")
    del buf, dst, direct_buf

    # 3: the noise stage alone
    fs, sigma = 2.6e6, 1000.0
    d0 = synth_blocks(NB, 1, seed=88)
    d0["prn"][:, 0] = 7
    d0["gain"][:, 0] = 0.0
    ctx.set_noise(SEED, sigma, 0)
    buf, n = render(ctx, d0, fs, SC16)
    for nfft in (64, 512):
        dens, navg = density(ctx, buf, n, SC16, nfft, fs)
        rel = dens / (2.0 * sigma * sigma / fs)
        lines.append(f"3 | noise stage, sigma {sigma:.0f}, gain-0 channel, int16, 2.6 Msps, nfft {nfft} ({navg} segments) | mean density / (2 sigma^2 / fs) {rel.mean():.5f} | "
                     f"over the bins: min {rel.min():.4f}, max {rel.max():.4f}, standard deviation {rel.std():.4f} (1 / sqrt(segments) = {1 / math.sqrt(navg):.4f})")
    del buf

    # 4: qmax 1 against qmax 127
    cn0, gain = 45.0, 2.0
    d["gain"][:, 0] = gain
    sigma = gpsiq.noise_sigma_for_cn0(cn0, gain, fs)
    ctx.set_noise(SEED, sigma, 0)
    rows = {}
    for qmax, share in ((127, 1 / 3.0), (1, 1.0)):
        ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms([gain], sigma), qmax * share), qmax)
        buf, n = render(ctx, d, fs, SC08)
        dens, navg = density(ctx, buf, n, SC08, 512, fs)
        x = buf.view(torch.int8).to(torch.float32)
        ms = float((x * x).mean())                                    # mean square per component
        rows[qmax] = dens / (2.0 * ms / fs)
        del buf, x
    f = freqs(512, fs)
    inband = np.abs(f) < 1.0e6
    lines.append(f"4 | one channel at {cn0:.0f} dB-Hz, int8, 2.6 Msps, nfft 512 ({navg} segments), density / (2 mean square / fs) | "
                 + " | ".join(f"qmax {q}: mean {r.mean():.4f}, min {r.min():.4f}, max {r.max():.4f}, |f| < 1 MHz against the rest {db(float(r[inband].mean()) / float(r[~inband].mean())):+.3f} dB"
                              for q, r in rows.items())
                 + f" | bin by bin qmax 1 / qmax 127: {db(float((rows[1] / rows[127]).min())):+.3f} to {db(float((rows[1] / rows[127]).max())):+.3f} dB")
    ctx.noise_off()
    ctx.level_off()

    # 5: the table-rounding floor
    c, s = (np.asarray(t, np.int64) for t in gpsiq.carrier_table())
    for nfft in (64, 512):
        k0 = nfft // 8 + 1
        idx = (k0 * np.arange(nfft * 64) * (512 // nfft)) % 512
        tone = np.stack([c[idx] * 131, s[idx] * 131], axis=1).astype(np.int16)          # 250 * 131 = 32750
        t = torch.from_numpy(tone.view(np.uint8).ravel().copy()).cuda()
        cols = []
        for window, name, skip in ((WINDOW_RECT, "rect", 0), (WINDOW_HANN, "hann", 1)):
            navg = gpsiq.spectrum_span(len(tone), nfft, nfft, 1)[0]
            shift = gpsiq.spectrum_min_shift(SC16, nfft, window, navg)
            p = ctx.spectrum(len(tone), SC16, t.data_ptr(), nfft, nfft, window, navg, shift)[0].astype(np.float64)
            other = np.ones(nfft, bool)
            other[[(k0 + j) % nfft for j in range(-skip, skip + 1)]] = False
            cols.append(f"{name}: bins other than the tone's{' and its two neighbours' if skip else ''}, largest {db(max(float(p[other].max()), 1.0) / float(p[k0])):+.1f} dB, "
                        f"mean {db(max(float(p[other].mean()), 1e-3) / float(p[k0])):+.1f} dB")
        lines.append(f"5 | table tone at bin {k0} of {nfft}, amplitude 32750, int16, {navg} segments without overlap, against the tone's bin | " + " | ".join(cols)
                     + f" | the estimate 1 / (12 * 250^2 * N): {db(1.0 / (12.0 * 62500.0 * nfft)):+.1f} dB")
    ctx.close()
    with open(out, "w") as fo:
        fo.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
