"""profiles/agc_signal.txt: what gpsiq_agc does to a receiver's C/N0 -- measured values, written down, not thresholds.  One channel at
45 dB-Hz (gain 1), 2.6 Msps, 64 blocks of 66 560 samples rendered as int16 with noise and no level; every figure is gpsiq_cn0_estimate on
gpsiq_despread's sums, and every loss is against the int16 stream before the stage.  Window 1024, navg 16, the first multiplier the one
gpsiq_level_mult gives for the floor, so the stage is level from its first window.
  1  the stage into int8 at qmax 1 and qmax 7 over a sweep of target_q8: the quantisation loss, and the target at which it is least
  2  a CW jammer from gpsiq_mix at J/S 20, 30 and 40 dB (against the satellite's amplitude of 250) that comes on half way through: the
     multiplier in the last window before it and in the last window of the run, and the C/N0 of the second half behind the stage
     against the same stream behind a FIXED multiplier -- the stage with mult_min = mult_max = the floor's multiplier, which is the
     arithmetic of gpsiq_set_level on this stream -- both against the jammed int16 stream itself
  3  a pulsed interferer (the J/S 40 dB tone gated on for 260 samples in 26 000) with the blanker off and on (threshold 6 sigma of the
     floor, hold 64)
usage: timeout -k 10 420 python scripts/agc_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import MIX_TONE, SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NB, NS, SEG, CN0, G = 2.6e6, 64, 66560, 2560, 45.0, 1.0
W, M = 1024, 16
T = gpsiq.MixTerm
SWEEP = {1: (0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.2, 1.5, 2.0), 7: (1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 5.0, 6.0)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "agc_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# python scripts/agc_signal.py: C/N0 through render, gpsiq_agc and gpsiq_despread, {FS / 1e6} Msps, {NB} blocks of {NS} samples, "
             f"one channel at {CN0} dB-Hz, window {W}, navg {M}, kernel id {gpsiq.kernels_id()}"]
    d = synth_blocks(NB, 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = 7, 19
    d["gain"][:, 0], d["gain"][:, 1] = G, 0.0
    ctx.set_descriptors(gpsiq.quantize_blocks(d, FS, NS)[0])
    sigma = gpsiq.noise_sigma_for_cn0(CN0, G, FS)
    floor = gpsiq.composite_rms([G], sigma)
    n = NB * NS
    clean = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    buf = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    ctx.set_noise(0xC0DE45, sigma, 0)
    ctx.launch(0, NB, NS, SC16, clean.data_ptr(), 4 * NS, stream=s)
    ctx.synchronize(s)

    def cn0(ptr, ss, b0=0, nb=NB):
        sums = ctx.despread(b0, nb, NS, ss, ptr + b0 * 2 * NS * ss, 2 * NS * ss, SEG, stream=s)[0]
        return gpsiq.cn0_estimate(sums[:, 0], SEG, FS)

    def stage(src, qmax, target, thresh=0, hold=0, fixed=None):
        """the int16 stream at src through the stage into dst -> (clipped, blanked, mults)"""
        m0 = gpsiq.level_mult(floor, target) if fixed is None else fixed
        cfg = gpsiq.AgcCfg(window=W, navg=M, target_q8=int(round(256 * target)), mult0=m0, mult_min=1 if fixed is None else fixed,
                           mult_max=(1 << 24) - 1 if fixed is None else fixed, blank_thresh=thresh, blank_hold=hold, qmax=qmax)
        return ctx.agc(n, SC16, src.data_ptr(), cfg, SC08, dst.data_ptr(), state=gpsiq.AgcState(), stream=s)[:3]

    a, sa = cn0(clean.data_ptr(), SC16)
    lines.append(f"int16 stream before the stage | C/N0 {a:.3f} dB-Hz, one sigma {sa:.3f} | rms per component {floor:.1f}")
    best = {}
    for qmax, targets in SWEEP.items():
        for target in targets:
            clipped, _, mults = stage(clean, qmax, target)
            b, sb = cn0(dst.data_ptr(), SC08)
            lines.append(f"qmax {qmax} | target rms {target:.2f} | multiplier {int(mults[M:].min())}..{int(mults.max())} | clipped {clipped / (2 * n):.4f} of the elements | "
                         f"C/N0 {b:.3f} | loss {b - a:+.3f} dB | one sigma {sb:.3f}")
            if qmax not in best or b > best[qmax][1]:
                best[qmax] = (target, b)
        lines.append(f"qmax {qmax} | least loss {best[qmax][1] - a:+.3f} dB at a target rms of {best[qmax][0]:.2f}")
    half, nhalf = NB // 2, (NB // 2) * NS
    for js in (20.0, 30.0, 40.0):
        buf.copy_(clean)
        step = gpsiq.mix_tone(FS, 100e3)[0]
        tone = T.tone(gpsiq.mix_gain(250.0 * G * 10.0 ** (js / 20.0), MIX_TONE, 0), step)
        second = buf.data_ptr() + 4 * nhalf
        jclip, _ = ctx.mix(nhalf, nhalf, [T.stream(second, SC16, 1), tone], 0, 32767, SC16, second, stream=s)
        j, _ = cn0(buf.data_ptr(), SC16, half, NB - half)
        for qmax in (1, 7):
            target = best[qmax][0]
            _, _, mults = stage(buf, qmax, target)
            g, _ = cn0(dst.data_ptr(), SC08, half, NB - half)
            fixed = gpsiq.level_mult(floor, target)
            fclip, _, _ = stage(buf, qmax, target, fixed=fixed)
            f, _ = cn0(dst.data_ptr(), SC08, half, NB - half)
            lines.append(f"CW jammer J/S {js:.0f} dB on from block {half} ({jclip} int16 elements clipped by the mix) | qmax {qmax}, target {target:.2f} | "
                         f"multiplier {int(mults[nhalf // W - 1])} before, {int(mults[-1])} at the end | second half: int16 {j:.3f} dB-Hz | "
                         f"behind the stage {g:.3f} ({g - j:+.3f} dB) | behind the fixed multiplier {fixed}: {f:.3f} ({f - j:+.3f} dB)")
    buf.copy_(clean)
    tone = T.tone(gpsiq.mix_gain(250.0 * G * 100.0, MIX_TONE, 0), gpsiq.mix_tone(FS, 100e3)[0], gate=(26000, 260, 0))
    ctx.mix(n, 0, [T.stream(buf.data_ptr(), SC16, 1), tone], 0, 32767, SC16, buf.data_ptr(), stream=s)
    p, _ = cn0(buf.data_ptr(), SC16)
    for qmax in (1, 7):
        target = best[qmax][0]
        for thresh, hold in ((0, 0), (int(6 * floor), 64)):
            _, blanked, mults = stage(buf, qmax, target, thresh, hold)
            b, _ = cn0(dst.data_ptr(), SC08)
            lines.append(f"pulsed interferer, J/S 40 dB, 260 samples in 26000 | int16 {p:.3f} dB-Hz | qmax {qmax}, target {target:.2f} | blanker "
                         f"{'off' if not thresh else f'threshold {thresh}, hold {hold}'} | blanked {blanked / n:.4f} of the samples | multiplier {int(mults[M:].min())}.."
                         f"{int(mults.max())} | C/N0 {b:.3f} ({b - a:+.3f} dB against the clean int16 stream)")
    ctx.noise_off()
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
