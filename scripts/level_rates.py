"""profiles/level_rates.txt: what the output level stage costs the synthesis kernel.  gpsiq_launch on resident descriptors, timed
with noise only (sigma 1000: the noise kernel, the yardstick) and with noise and level (the level kernel), for int8 and int16 at
2.6 Msps and int16 at 25 Msps, 16 channels, 4 130 blocks' worth of samples per launch at 2.6 Msps int8 (about 2 GB of output per
launch in every configuration: the int16 rows halve the block count, the 25 Msps row divides it by the rate); then level on with
noise off (the level kernel drawing from the all-zero table) against both off, which is what that combination pays.
usage: timeout -k 10 240 python scripts/level_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

CONFIGS = [("2.6 Msps int8 16 ch 4130 blocks (headline)", 2.6e6, SC08, 4130),
           ("2.6 Msps int16 16 ch 2065 blocks", 2.6e6, SC16, 2065),
           ("25 Msps int16 16 ch 215 blocks", 25e6, SC16, 215)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "level_rates.txt")
    ctx = gpsiq.Context(0)
    lines = [f"# output level: gpsiq_launch (default variant) on resident descriptors, kernel id {gpsiq.kernels_id()}; sigma 1000, level = rms at a third of full scale",
             "# config | both off ms | noise only ms | noise + level ms | level alone ms | noise only G samples/s | noise + level G samples/s | level on / noise only (rate) | level alone / noise only | level alone / both off"]
    for name, fs, ss, nb in CONFIGS:
        nsamp = int(round(fs / 10))
        desc = synth_blocks(nb, 16, seed=1)
        q = gpsiq.quantize_blocks(desc, fs, nsamp)[0]
        ctx.set_descriptors(q)
        stride = 2 * nsamp * ss
        buf = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        qmax = 127 if ss == SC08 else 32767
        lv = (gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], 1000.0), qmax / 3.0), qmax)
        res = []
        for sigma, level in ((1000.0, None), (1000.0, lv), (0.0, lv), (0.0, None)):
            ctx.set_noise(7, sigma, 0)
            if level:
                ctx.set_level(*level)
            else:
                ctx.level_off()
            ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 3, stream=s)               # warm-up
            res.append(min(ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 10, stream=s) for _ in range(5)))
        ctx.level_off()
        gs = [nb * nsamp / (m * 1e-3) / 1e9 for m in res]
        lines.append(f"{name} | {res[3]:.3f} | {res[0]:.3f} | {res[1]:.3f} | {res[2]:.3f} | {gs[0]:.1f} | {gs[1]:.1f} | {res[0] / res[1]:.3f} | {res[0] / res[2]:.3f} | {res[3] / res[2]:.3f}")
        del buf
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
