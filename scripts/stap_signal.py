"""profiles/stap_signal.txt: what taps behind two elements give back of a receiver's C/N0 under a broadband jammer that arrives twice
-- directly, and again D samples later from another direction, the reflection -- measured values, written down, not thresholds.  Two
elements; one channel at 45 dB-Hz (gain 0.2, amplitude 50, so that a jammer 50 dB above it and its echo still fit int16), 2.6 Msps, 64
blocks of 66 560 samples rendered per element as int16 with the element's phase on the carrier (gpsiq.array_element) and a noise seed
of its own.  gpsiq_mix adds a chirp (the whole band every 1 021 samples) at J/S 30, 40 and 50 dB and the same chirp D samples late at
0.7 of its amplitude (the sweep's offset and phase0 moved by D samples), each at its own phase per element.  Then, per row:
  one element                   element 0 as it is
  two elements, spatial         gpsiq_stap_cov and gpsiq_stap_weights with one tap, gpsiq_stap_combine
  two elements, four taps       the same with four taps
each by power inversion and steered at the satellite, no loading; and for every stream gpsiq_agc into int8 at qmax 1 and at qmax 7
(window 1024, navg 16, the first multiplier the one gpsiq_level_mult gives for the stream's own measured rms), gpsiq_despread against
element 0's descriptors and gpsiq_cn0_estimate.
usage: timeout -k 10 420 python scripts/stap_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import MIX_TONE, SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NB, NS, SEG, CN0, G = 2.6e6, 64, 66560, 2560, 45.0, 0.2
W, M = 1024, 16
PERIOD, D, ECHO = 1021, 2, 0.7
NELEM, NTAPS = 2, 4
TARGET = {1: 0.9, 7: 3.0}
SAT = np.array([0.0, 0.37])                 # the satellite's phase at the elements, cycles
DIRECT, REFLECTED = np.array([0.0, 0.25]), np.array([0.11, 0.002])      # the jammer's two arrivals
T = gpsiq.MixTerm


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stap_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# python scripts/stap_signal.py: C/N0 through render, gpsiq_mix, gpsiq_stap_cov, gpsiq_stap_weights, gpsiq_stap_combine, gpsiq_agc and gpsiq_despread, "
             f"{FS / 1e6} Msps, {NB} blocks of {NS} samples, two elements, one channel at {CN0} dB-Hz (gain {G}) at phases {SAT.tolist()} cycles, a chirp over the whole band "
             f"every {PERIOD} samples at phases {DIRECT.tolist()} and again {D} samples later at {ECHO} of its amplitude at phases {REFLECTED.tolist()}, kernel id {gpsiq.kernels_id()}"]
    d = synth_blocks(NB, 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = 7, 19
    d["gain"][:, 0], d["gain"][:, 1] = G, 0.0
    sigma = gpsiq.noise_sigma_for_cn0(CN0, G, FS)
    n = NB * NS
    clean = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(NELEM)]
    jam = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(NELEM)]
    y = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    q8 = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    q0 = None
    for e in range(NELEM):
        q = gpsiq.quantize_blocks(gpsiq.array_element(d, [SAT[e], SAT[e]]), FS, NS)[0]
        q0 = q if e == 0 else q0
        ctx.set_noise(0xC0DE45 + e, sigma, 0)
        ctx.set_descriptors(q)
        ctx.launch(0, NB, NS, SC16, clean[e].data_ptr(), 4 * NS, stream=s)
        ctx.synchronize(s)
    ctx.noise_off()
    ctx.set_descriptors(q0)                                           # the correlator's replica: element 0's timeline

    def cn0(t, ss):
        sums = ctx.despread(0, NB, NS, ss, t.data_ptr(), 2 * NS * ss, SEG, stream=s)[0]
        return gpsiq.cn0_estimate(sums[:, 0], SEG, FS)[0]

    def rms(t):
        return float(t.view(torch.int16).to(torch.float64).square().mean().sqrt().item())

    def quantised(t, qmax):
        target = TARGET[qmax]
        cfg = gpsiq.AgcCfg(window=W, navg=M, target_q8=int(round(256 * target)), mult0=gpsiq.level_mult(rms(t), target), qmax=qmax)
        ctx.agc(n, SC16, t.data_ptr(), cfg, SC08, q8.data_ptr(), state=gpsiq.AgcState(), stream=s)
        return cn0(q8, SC08)

    def row(t):
        return cn0(t, SC16), quantised(t, 1), quantised(t, 7)

    base = row(clean[0])
    lines.append(f"clean, element 0 alone | int16 {base[0]:.3f} dB-Hz | qmax 1 {base[1]:.3f} | qmax 7 {base[2]:.3f} | rms per component {rms(clean[0]):.1f}")
    step, rate = -(1 << 58), (1 << 59) // PERIOD
    for js in (30.0, 40.0, 50.0):
        amp = 250.0 * G * 10.0 ** (js / 20.0)
        gain, egain = gpsiq.mix_gain(amp, MIX_TONE, 0), gpsiq.mix_gain(ECHO * amp, MIX_TONE, 0)
        jclip = 0
        for e in range(NELEM):
            first = T.tone(gain, step, phase0=int(round(DIRECT[e] * 2 ** 59)) % 2 ** 64, rate=rate, sweep=(PERIOD, 0))
            # the same chirp D samples late: the sweep's clock and the carrier's phase both moved back by D samples
            late = T.tone(egain, step, phase0=(int(round(REFLECTED[e] * 2 ** 59)) - D * step) % 2 ** 64, rate=rate, sweep=(PERIOD, PERIOD - D))
            jclip += ctx.mix(n, 0, [T.stream(clean[e].data_ptr(), SC16, 1), first, late], 0, 32767, SC16, jam[e].data_ptr(), stream=s)[0]
        ptrs = [t.data_ptr() for t in jam]
        j = row(jam[0])
        lines.append(f"J/S {js:.0f} dB (chirp amplitude {250 * gain}, echo {250 * egain}) | one element | int16 {j[0]:.3f} dB-Hz ({j[0] - base[0]:+.3f}) | "
                     f"qmax 1 {j[1]:.3f} ({j[1] - base[1]:+.3f}) | qmax 7 {j[2]:.3f} ({j[2] - base[2]:+.3f}) | rms {rms(jam[0]):.1f} | {jclip} int16 elements clamped by the mix")
        for ntaps in (1, NTAPS):
            cov, cms = ctx.stap_cov(ptrs, n, SC16, ntaps, stream=s)
            kernel = ctx.stap_last_plan()[0]
            for name, steer in (("power inversion", None), ("steered", SAT)):
                for shift in range(13, 5, -1):                        # the caller lowers shift while the weights do not fit
                    try:
                        w = gpsiq.stap_weights(cov, n, NELEM, ntaps, steer=steer, ref_tap=0, loading=0.0, shift=shift)
                        break
                    except gpsiq.GpsiqError as err:
                        refused = err
                else:                                                 # no shift fits: a row with another row's weights would be wrong
                    raise refused
                clipped, ms = ctx.stap_combine(ptrs, n, SC16, w, shift, SC16, y.data_ptr(), stream=s)
                v = row(y)
                lines.append(f"J/S {js:.0f} dB | {NELEM} x {ntaps} {name} | int16 {v[0]:.3f} dB-Hz ({v[0] - base[0]:+.3f} against clean, {v[0] - j[0]:+.3f} over one element) | "
                             f"qmax 1 {v[1]:.3f} ({v[1] - base[1]:+.3f}, {v[1] - j[1]:+.3f}) | qmax 7 {v[2]:.3f} ({v[2] - base[2]:+.3f}, {v[2] - j[2]:+.3f}) | rms {rms(y):.1f} | "
                             f"weights over 2^{shift}: {w.reshape(-1, 2).tolist()} | stap_cov {kernel} {cms:.3f} ms, stap_combine {ms:.3f} ms, {clipped} elements clamped")
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
