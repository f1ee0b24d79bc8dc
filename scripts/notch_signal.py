"""profiles/notch_signal.txt: what a notch in front of the quantiser gives back of a receiver's C/N0 under a CW jammer -- measured values,
written down, not thresholds.  One channel at 45 dB-Hz (gain 1), 2.6 Msps, 64 blocks of 66 560 samples rendered as int16 with noise
and no level.  gpsiq_mix adds a CW jammer at +100 kHz at J/S 20, 30 and 40 dB (against the satellite's amplitude of 250) over the
whole run.  Then, optionally, the notch: gpsiq_spectrum (nfft 256, Hann, hop 128, one group) -> gpsiq_notch_find at ratio 8 ->
gpsiq_notch_design (129 taps, 4 bins wide, shift 12) -> gpsiq_cfilter int16 to int16.  Then gpsiq_agc into int8 at qmax 1 and at qmax 7
(window 1024, navg 16, the first multiplier the one gpsiq_level_mult gives for the stream's own measured rms), gpsiq_despread and
gpsiq_cn0_estimate.  Reported per J/S and qmax: C/N0 clean, jammed and notched behind the same quantiser, and the notched stream's
loss against the clean one.
The filter delays the stream by c = 64 samples: the notched stream is despread from 64 samples further on, so that its block b
starts at the sample the descriptors of block b describe; and every stream is measured over blocks 1 .. 62 -- the first block holds
the filter's start-up from a zero history (128 samples), the last is the one the shifted stream no longer fills.
usage: timeout -k 10 420 python scripts/notch_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import MIX_TONE, SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NB, NS, SEG, CN0, G = 2.6e6, 64, 66560, 2560, 45.0, 1.0
W, M = 1024, 16
NFFT, HOP, RATIO = 256, 128, 8.0
NTAPS, WIDTH_BINS, SHIFT = 129, 4, 12
F_JAM = 100e3
TARGET = {1: 0.9, 7: 3.0}
T = gpsiq.MixTerm


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "notch_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# python scripts/notch_signal.py: C/N0 through render, gpsiq_mix, the notch (gpsiq_spectrum, gpsiq_notch_find, gpsiq_notch_design, gpsiq_cfilter), "
             f"gpsiq_agc and gpsiq_despread, {FS / 1e6} Msps, {NB} blocks of {NS} samples, one channel at {CN0} dB-Hz, CW at {F_JAM / 1e3:+.0f} kHz, "
             f"{NTAPS} taps, {WIDTH_BINS} bins of {NFFT} wide, shift {SHIFT}, kernel id {gpsiq.kernels_id()}"]
    d = synth_blocks(NB, 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = 7, 19
    d["gain"][:, 0], d["gain"][:, 1] = G, 0.0
    ctx.set_descriptors(gpsiq.quantize_blocks(d, FS, NS)[0])
    sigma = gpsiq.noise_sigma_for_cn0(CN0, G, FS)
    n, c = NB * NS, (NTAPS - 1) // 2
    clean = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    jam = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    notched = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    q8 = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    ctx.set_noise(0xC0DE45, sigma, 0)
    ctx.launch(0, NB, NS, SC16, clean.data_ptr(), 4 * NS, stream=s)
    ctx.synchronize(s)
    b0, nb = 1, NB - 2

    def cn0(t, ss, skip=0):
        """C/N0 of blocks b0 .. b0 + nb - 1 of the stream in t, block b taken from sample b * NS + skip on"""
        sums = ctx.despread(b0, nb, NS, ss, t.data_ptr() + (b0 * NS + skip) * 2 * ss, 2 * NS * ss, SEG, stream=s)[0]
        return gpsiq.cn0_estimate(sums[:, 0], SEG, FS)[0]

    def rms(t):
        return float(t.view(torch.int16).to(torch.float64).square().mean().sqrt().item())

    def quantised(t, qmax, skip=0):
        """the int16 stream in t through gpsiq_agc into int8 at qmax -> (C/N0, elements clamped / all)"""
        target = TARGET[qmax]
        cfg = gpsiq.AgcCfg(window=W, navg=M, target_q8=int(round(256 * target)), mult0=gpsiq.level_mult(rms(t), target), qmax=qmax)
        clipped = ctx.agc(n, SC16, t.data_ptr(), cfg, SC08, q8.data_ptr(), state=gpsiq.AgcState(), stream=s)[0]
        return cn0(q8, SC08, skip), clipped / (2 * n)

    a16 = cn0(clean, SC16)
    lines.append(f"int16 clean stream | C/N0 {a16:.3f} dB-Hz | rms per component {rms(clean):.1f}")
    base = {}
    for qmax in (1, 7):
        base[qmax], clip = quantised(clean, qmax)
        lines.append(f"clean | qmax {qmax}, target {TARGET[qmax]:.2f} | C/N0 {base[qmax]:.3f} dB-Hz ({base[qmax] - a16:+.3f} dB against int16) | clamped {clip:.4f} of the elements")
    for js in (20.0, 30.0, 40.0):
        tone = T.tone(gpsiq.mix_gain(250.0 * G * 10.0 ** (js / 20.0), MIX_TONE, 0), gpsiq.mix_tone(FS, F_JAM)[0])
        jclip, _ = ctx.mix(n, 0, [T.stream(clean.data_ptr(), SC16, 1), tone], 0, 32767, SC16, jam.data_ptr(), stream=s)
        power = ctx.spectrum(n, SC16, jam.data_ptr(), NFFT, hop=HOP, window=1, stream=s)
        f, ex, nl = gpsiq.notch_find(power[0], FS, RATIO, 8)
        found = ", ".join(f"{fi / 1e3:+.3f} kHz at {ei:.1f} dB" for fi, ei in zip(f, ex))
        lines.append(f"J/S {js:.0f} dB | {jclip} int16 elements clamped by the mix | rms {rms(jam):.1f} | lines found: {nl} ({found})")
        j16 = cn0(jam, SC16)
        if nl:
            taps = gpsiq.notch_design(FS, f, WIDTH_BINS * FS / NFFT, NTAPS, SHIFT)
            _, fclip, ms = ctx.cfilter(n, SC16, jam.data_ptr(), taps, SHIFT, 1, 0, SC16, notched.data_ptr(), stream=s)
            n16 = cn0(notched, SC16, c)
            after = gpsiq.notch_find(ctx.spectrum(n, SC16, notched.data_ptr(), NFFT, hop=HOP, window=1, stream=s)[0], FS, RATIO, 8)[2]
            lines.append(f"J/S {js:.0f} dB | int16: jammed {j16:.3f} dB-Hz ({j16 - a16:+.3f}) | notched {n16:.3f} ({n16 - a16:+.3f} against clean) | "
                         f"gpsiq_cfilter {ctx.cfilter_last_plan()[0]} {ms:.3f} ms, {fclip} elements clamped | rms {rms(notched):.1f} | lines left: {after}")
        for qmax in (1, 7):
            j, jc = quantised(jam, qmax)
            row = f"J/S {js:.0f} dB | qmax {qmax} | clean {base[qmax]:.3f} dB-Hz | jammed {j:.3f} ({j - base[qmax]:+.3f})"
            if nl:
                v, vc = quantised(notched, qmax, c)
                row += f" | notched {v:.3f} | loss of the notched stream against the clean one {v - base[qmax]:+.3f} dB | gained over the jammed one {v - j:+.3f} dB"
            lines.append(row)
    ctx.noise_off()
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
