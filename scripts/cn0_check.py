"""profiles/despread_cn0.txt: does a stream rendered at a set C/N0 hold that C/N0?  One channel at gain 2 and a gain-0 probe, 2.6 Msps,
64 blocks of 66 560 samples (1 664 segments of 2 560), noise at gpsiq_noise_sigma_for_cn0(set, 2, fs): rendered by gpsiq_launch,
despread by gpsiq_despread from the same device stream, estimated by gpsiq_cn0_estimate.  Rows: int16 without level, int8 with the
level at a third of full scale (qmax 127), qmax 7 and qmax 1 (int8 container, rms at a third of the clamp; for qmax 1 at the clamp),
each at 40 / 45 / 50 dB-Hz; for the levelled rows the counted share of elements at the clamp beside the share a Gaussian of the
composite rms puts there.  Measured values, written down: not thresholds.
usage: timeout -k 10 300 python scripts/cn0_check.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NSAMP, NB, SEG, GAIN, SEED = 2.6e6, 66560, 64, 2560, 2.0, 0xC0DE45
# (name, format, qmax, rms of the output as a share of qmax); None: no level
ROWS = [("int16, no level", SC16, None, None), ("int8, level at qmax/3, qmax 127", SC08, 127, 1 / 3.0),
        ("int8 container, qmax 7, level at qmax/3", SC08, 7, 1 / 3.0), ("int8 container, qmax 1, level at qmax", SC08, 1, 1.0)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "despread_cn0.txt")
    ctx = gpsiq.Context(0)
    d = synth_blocks(NB, 2, seed=45)
    d["prn"][:, 0], d["prn"][:, 1] = 7, 19
    d["gain"][:, 0], d["gain"][:, 1] = GAIN, 0.0
    q = gpsiq.quantize_blocks(d, FS, NSAMP)[0]
    ctx.set_descriptors(q)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# python scripts/cn0_check.py: one channel at gain {GAIN} + a gain-0 probe, {FS / 1e6} Msps, {NB} blocks of {NSAMP} samples, {NB * NSAMP // SEG} segments of {SEG}; kernel id {gpsiq.kernels_id()}",
             "# stream | set dB-Hz | measured dB-Hz | one_sigma_db | measured - set | probe mean / its standard error | counted share of |x| >= qmax (I, Q) | predicted share 2 Q(qmax - 1/2 over rms)"]
    for name, ss, qmax, share in ROWS:
        for cn0 in (40.0, 45.0, 50.0):
            sigma = gpsiq.noise_sigma_for_cn0(cn0, GAIN, FS)
            ctx.set_noise(SEED, sigma, 0)
            pred = ""
            if qmax is None:
                ctx.level_off()
            else:
                rms_in, rms_out = gpsiq.composite_rms([GAIN], sigma), qmax * share
                ctx.set_level(gpsiq.level_mult(rms_in, rms_out), qmax)
                # an element reaches the clamp when the scaled value rounds to qmax or beyond: |y| >= qmax - 1/2
                pred = f"{math.erfc((qmax - 0.5) / rms_out / math.sqrt(2.0)):.5f}"
            stride = 2 * NSAMP * ss
            buf = torch.empty(NB * stride, dtype=torch.uint8, device="cuda")
            ctx.launch(0, NB, NSAMP, ss, buf.data_ptr(), stride, stream=s)
            sums, prn, st, _ = ctx.despread(0, NB, NSAMP, ss, buf.data_ptr(), stride, SEG, clip=qmax or 32767, stream=s)
            got, one = gpsiq.cn0_estimate(sums[:, 0], SEG, FS)
            p = sums["i"][:, 1].astype(float).ravel()
            probe = p.mean() / (p.std(ddof=1) / math.sqrt(p.size))
            n = NB * NSAMP
            clip = f"{st['clip_i'].sum() / n:.5f}, {st['clip_q'].sum() / n:.5f}" if qmax else "-"
            lines.append(f"{name} | {cn0:.0f} | {got:.3f} | {one:.3f} | {got - cn0:+.3f} | {probe:+.2f} | {clip} | {pred or '-'}")
            del buf
    ctx.noise_off()
    ctx.level_off()
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
