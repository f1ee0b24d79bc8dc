"""profiles/stap_beams_signal.txt: what one beam per satellite gives a receiver that one steered beam does not -- measured values,
written down, not thresholds.  Four elements on a half-wavelength square; four satellites from four directions in four channel slots,
each at 45 dB-Hz (gain 0.2, amplitude 50, so that a jammer 50 dB above one of them and its echo still fit int16), 2.6 Msps, 64 blocks
of 66 560 samples rendered per element as int16 with the element's phases on the carriers (gpsiq.array_steer, gpsiq.array_element)
and a noise seed of its own.  gpsiq_mix adds a chirp (the whole band every 1 021 samples) at J/S 30, 40 and 50 dB from one direction
and the same chirp D samples late at 0.7 of its amplitude from another (scripts/stap_signal.py's jammer, with directions).  Then
gpsiq_stap_cov over four taps, gpsiq_stap_beam_weights towards the four satellites (no loading), and ONE gpsiq_stap_beams call for the
four beams.  Per row and satellite the C/N0 by gpsiq_despread against element 0's descriptors and gpsiq_cn0_estimate, for the int16
stream and behind gpsiq_agc into int8 at qmax 1 and at qmax 7 (window 1024, navg 16, the first multiplier the one gpsiq_level_mult
gives for the stream's own measured rms):
  clean element          element 0 before the jammer
  jammed element         element 0 as it is
  beam at satellite 0    every satellite behind the beam steered at satellite 0: what one gpsiq_stap_combine call gives a receiver
  own beam               every satellite behind the beam steered at it
`nan`: the satellite's mean prompt is not positive behind that stream, and gpsiq_cn0_estimate refuses to rate it: the satellite is lost.
usage: timeout -k 10 420 python scripts/stap_beams_signal.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import math
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
PERIOD, D, ECHO = 1021, 3, 0.7
NELEM, NTAPS = 4, 4
TARGET = {1: 0.9, 7: 3.0}
SQUARE = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.5, 0.5, 0.0]])
PRNS = (7, 19, 3, 28)
SATS = ((30.0, 50.0), (120.0, 35.0), (210.0, 65.0), (300.0, 25.0))      # azimuth, elevation in degrees
JAM_DIRECT, JAM_ECHO = (75.0, 5.0), (250.0, 12.0)
T = gpsiq.MixTerm


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stap_beams_signal.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    rad = math.pi / 180.0
    steers = np.stack([gpsiq.array_steer(SQUARE, az * rad, el * rad) for az, el in SATS])            # [satellite, element]
    direct, reflected = (gpsiq.array_steer(SQUARE, az * rad, el * rad) for az, el in (JAM_DIRECT, JAM_ECHO))
    nsat = len(PRNS)
    lines = [f"# python scripts/stap_beams_signal.py: C/N0 per satellite through render, gpsiq_mix, gpsiq_stap_cov, gpsiq_stap_beam_weights, ONE gpsiq_stap_beams call, "
             f"gpsiq_agc and gpsiq_despread, {FS / 1e6} Msps, {NB} blocks of {NS} samples, four elements on a half-wavelength square, {NTAPS} taps, PRNs {list(PRNS)} at "
             f"{CN0} dB-Hz (gain {G}) from (az, el) {list(SATS)} degrees, a chirp over the whole band every {PERIOD} samples from {JAM_DIRECT} and again {D} samples later at "
             f"{ECHO} of its amplitude from {JAM_ECHO}, kernel id {gpsiq.kernels_id()}",
             "# every row: what | satellite (PRN) | int16 dB-Hz | behind qmax 1 | behind qmax 7   (in brackets: against the clean element's figure of the same column)"]
    d = synth_blocks(NB, nsat, seed=45)
    for k, prn in enumerate(PRNS):
        d["prn"][:, k], d["gain"][:, k] = prn, G
    sigma = gpsiq.noise_sigma_for_cn0(CN0, G, FS)
    n = NB * NS
    clean = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(NELEM)]
    jam = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(NELEM)]
    ys = [torch.empty(4 * n, dtype=torch.uint8, device="cuda") for _ in range(nsat)]
    q8 = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    q0 = None
    for e in range(NELEM):
        q = gpsiq.quantize_blocks(gpsiq.array_element(d, steers[:, e]), FS, NS)[0]
        q0 = q if e == 0 else q0
        ctx.set_noise(0xC0DE45 + e, sigma, 0)
        ctx.set_descriptors(q)
        ctx.launch(0, NB, NS, SC16, clean[e].data_ptr(), 4 * NS, stream=s)
        ctx.synchronize(s)
    ctx.noise_off()
    ctx.set_descriptors(q0)                                           # the correlator's replicas: element 0's timeline, one slot per satellite

    def cn0(t, ss):
        sums = ctx.despread(0, NB, NS, ss, t.data_ptr(), 2 * NS * ss, SEG, stream=s)[0]
        return [estimate(sums[:, k]) for k in range(nsat)]

    def estimate(sums):
        try:
            return gpsiq.cn0_estimate(sums, SEG, FS)[0]
        except gpsiq.GpsiqError:                                     # the mean prompt is not positive: the estimator has no signal to rate
            return float("nan")

    def rms(t):
        return float(t.view(torch.int16).to(torch.float64).square().mean().sqrt().item())

    def quantised(t, qmax):
        target = TARGET[qmax]
        cfg = gpsiq.AgcCfg(window=W, navg=M, target_q8=int(round(256 * target)), mult0=gpsiq.level_mult(rms(t), target), qmax=qmax)
        ctx.agc(n, SC16, t.data_ptr(), cfg, SC08, q8.data_ptr(), state=gpsiq.AgcState(), stream=s)
        return cn0(q8, SC08)

    def table(t):
        """[satellite][column]: int16, qmax 1, qmax 7"""
        return np.array([cn0(t, SC16), quantised(t, 1), quantised(t, 7)]).T

    base = table(clean[0])
    for k in range(nsat):
        lines.append(f"clean element | {k} ({PRNS[k]}) | {base[k, 0]:.3f} | {base[k, 1]:.3f} | {base[k, 2]:.3f} | rms per component {rms(clean[0]):.1f}")

    def rows(what, tab, sats, tail=""):
        for k in sats:
            v = tab[k] if tab.ndim == 2 else tab
            lines.append(f"{what} | {k} ({PRNS[k]}) | " + " | ".join(f"{v[c]:.3f} ({v[c] - base[k, c]:+.3f})" for c in range(3)) + tail)

    step, rate = -(1 << 58), (1 << 59) // PERIOD
    for js in (30.0, 40.0, 50.0):
        amp = 250.0 * G * 10.0 ** (js / 20.0)
        gain, egain = gpsiq.mix_gain(amp, MIX_TONE, 0), gpsiq.mix_gain(ECHO * amp, MIX_TONE, 0)
        jclip = 0
        for e in range(NELEM):
            first = T.tone(gain, step, phase0=int(round(direct[e] * 2 ** 59)) % 2 ** 64, rate=rate, sweep=(PERIOD, 0))
            # the same chirp D samples late: the sweep's clock and the carrier's phase both moved back by D samples
            late = T.tone(egain, step, phase0=(int(round(reflected[e] * 2 ** 59)) - D * step) % 2 ** 64, rate=rate, sweep=(PERIOD, PERIOD - D))
            jclip += ctx.mix(n, 0, [T.stream(clean[e].data_ptr(), SC16, 1), first, late], 0, 32767, SC16, jam[e].data_ptr(), stream=s)[0]
        ptrs = [t.data_ptr() for t in jam]
        rows(f"J/S {js:.0f} dB | jammed element", table(jam[0]), range(nsat), f" | rms {rms(jam[0]):.1f} | chirp amplitude {250 * gain}, echo {250 * egain}, {jclip} int16 elements clamped by the mix")
        cov, cms = ctx.stap_cov(ptrs, n, SC16, NTAPS, stream=s)
        for shift in range(13, 5, -1):                                # the caller lowers shift while the weights do not fit
            try:
                w = gpsiq.stap_beam_weights(cov, n, NELEM, NTAPS, steers, ref_tap=0, loading=0.0, shift=shift)
                break
            except gpsiq.GpsiqError as err:
                refused = err
        else:
            raise refused
        clipped, ms = ctx.stap_beams(ptrs, n, SC16, w, shift, SC16, [y.data_ptr() for y in ys], stream=s)
        plan = ctx.stap_beams_last_plan()
        tabs = [table(y) for y in ys]
        rows(f"J/S {js:.0f} dB | beam at satellite 0", tabs[0], range(nsat), f" | rms {rms(ys[0]):.1f}")
        for b in range(nsat):
            rows(f"J/S {js:.0f} dB | own beam", tabs[b], [b], f" | rms {rms(ys[b]):.1f}")
        lines.append(f"# J/S {js:.0f} dB: weights over 2^{shift}, sum |re| + |im| per beam {np.abs(w.astype(np.int64)).reshape(nsat, -1).sum(axis=1).tolist()}; stap_cov {cms:.3f} ms, "
                     f"one stap_beams call ({plan[0]}) {ms:.3f} ms for {nsat} beams, elements clamped per beam {clipped.tolist()}")
    ctx.close()
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
