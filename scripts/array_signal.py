"""profiles/array_signal.txt: what a four-element array gives back of a receiver's C/N0 under a jammer the notch cannot touch -- a chirp
swept across the whole sampled band -- measured values, written down, not thresholds.  Four elements on a half-wavelength square; one
channel at 45 dB-Hz (gain 0.25, amplitude 62.5, so that a jammer 50 dB above it still fits int16), 2.6 Msps, 64 blocks of 66 560
samples rendered per element as int16 with the element's geometric phase on the carrier (gpsiq.array_element) and a noise seed of its
own.  gpsiq_mix adds the chirp (the whole band every 1 021 samples) at J/S 30, 40 and 50 dB, its phase0 per element from
gpsiq_array_steer.  Then gpsiq_array_cov over the four jammed streams, gpsiq_array_weights (no loading) once as power inversion and once
steered at the satellite, gpsiq_array_combine into int16, and for every stream gpsiq_agc into int8 at qmax 1 and at qmax 7 (window
1024, navg 16, the first multiplier the one gpsiq_level_mult gives for the stream's own measured rms), gpsiq_despread against element
0's descriptors and gpsiq_cn0_estimate.
usage: timeout -k 10 420 python scripts/array_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import MIX_TONE, SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NB, NS, SEG, CN0, G = 2.6e6, 64, 66560, 2560, 45.0, 0.25
W, M = 1024, 16
PERIOD = 1021
TARGET = {1: 0.9, 7: 3.0}
SQUARE = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.5, 0.5, 0.0]])
SAT_DIR, JAM_DIR = (0.3, 0.9), (2.0, 0.1)
T = gpsiq.MixTerm


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "array_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    sat, jam_ph = gpsiq.array_steer(SQUARE, *SAT_DIR), gpsiq.array_steer(SQUARE, *JAM_DIR)
    lines = [f"# python scripts/array_signal.py: C/N0 through render, gpsiq_mix, gpsiq_array_cov, gpsiq_array_weights, gpsiq_array_combine, gpsiq_agc and gpsiq_despread, "
             f"{FS / 1e6} Msps, {NB} blocks of {NS} samples, four elements on a half-wavelength square, one channel at {CN0} dB-Hz (gain {G}) from az {SAT_DIR[0]} el {SAT_DIR[1]} rad, "
             f"a chirp over the whole band every {PERIOD} samples from az {JAM_DIR[0]} el {JAM_DIR[1]} rad, kernel id {gpsiq.kernels_id()}",
             f"# satellite phases {np.round(sat, 4).tolist()} cycles, jammer phases {np.round(jam_ph, 4).tolist()} cycles"]
    d = synth_blocks(NB, 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = 7, 19
    d["gain"][:, 0], d["gain"][:, 1] = G, 0.0
    sigma = gpsiq.noise_sigma_for_cn0(CN0, G, FS)
    n = NB * NS
    clean = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(4)]
    jam = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(4)]
    y = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    q8 = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    q0 = None
    for e in range(4):
        q = gpsiq.quantize_blocks(gpsiq.array_element(d, [sat[e], sat[e]]), FS, NS)[0]
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
        gain = gpsiq.mix_gain(250.0 * G * 10.0 ** (js / 20.0), MIX_TONE, 0)
        jclip = 0
        for e in range(4):
            tone = T.tone(gain, step, phase0=int(round(jam_ph[e] * 2 ** 59)), rate=rate, sweep=(PERIOD, 0))
            jclip += ctx.mix(n, 0, [T.stream(clean[e].data_ptr(), SC16, 1), tone], 0, 32767, SC16, jam[e].data_ptr(), stream=s)[0]
        ptrs = [t.data_ptr() for t in jam]
        j = row(jam[0])
        lines.append(f"J/S {js:.0f} dB (chirp amplitude {250 * gain}) | element 0 jammed | int16 {j[0]:.3f} dB-Hz ({j[0] - base[0]:+.3f}) | qmax 1 {j[1]:.3f} ({j[1] - base[1]:+.3f}) | "
                     f"qmax 7 {j[2]:.3f} ({j[2] - base[2]:+.3f}) | rms {rms(jam[0]):.1f} | {jclip} int16 elements clamped by the mix")
        cov, cms = ctx.array_cov(ptrs, n, SC16, stream=s)
        kernel = ctx.array_last_plan()[0]
        for name, steer in (("power inversion", None), ("steered", sat)):
            for shift in range(13, 7, -1):                            # the caller lowers shift while the weights do not fit
                try:
                    w = gpsiq.array_weights(cov, n, steer=steer, loading=0.0, shift=shift)
                    break
                except gpsiq.GpsiqError:
                    continue
            clipped, ms = ctx.array_combine(ptrs, n, SC16, w, shift, SC16, y.data_ptr(), stream=s)
            v = row(y)
            lines.append(f"J/S {js:.0f} dB | {name} | int16 {v[0]:.3f} dB-Hz ({v[0] - base[0]:+.3f} against clean, {v[0] - j[0]:+.3f} over jammed) | qmax 1 {v[1]:.3f} ({v[1] - base[1]:+.3f}, "
                         f"{v[1] - j[1]:+.3f}) | qmax 7 {v[2]:.3f} ({v[2] - base[2]:+.3f}, {v[2] - j[2]:+.3f}) | rms {rms(y):.1f} | weights over 2^{shift}: {w.tolist()} | "
                         f"array_cov {kernel} {cms:.3f} ms, array_combine {ms:.3f} ms, {clipped} elements clamped")
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
