"""profiles/despread_rates.txt: what the device correlator (gpsiq_despread, include/gpsiq_rows.h) costs.  For 2.6 Msps int8 with
4 130 blocks, int16 with 2 065 and 25 Msps int16 with 215, all at 16 channels and seg_len 2 560: kernel_ms of gpsiq_despread (the
minimum of five calls, after a warm-up call), beside it, timed in the same run, the gpsiq_launch of the same blocks (the synthesis
kernel, which this feature leaves as it was) and the time the stream's bytes take at the HBM read roof (8 TB/s).  The stream the
correlator reads is the one that launch rendered.
usage: timeout -k 10 300 python scripts/despread_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

HBM_PEAK_GBS = 8000.0
SEG_LEN = 2560
CONFIGS = [("2.6 Msps int8 16 ch 4130 blocks (headline)", 2.6e6, SC08, 4130),
           ("2.6 Msps int16 16 ch 2065 blocks", 2.6e6, SC16, 2065),
           ("25 Msps int16 16 ch 215 blocks", 25e6, SC16, 215)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "despread_rates.txt")
    ctx = gpsiq.Context(0)
    lines = [f"# python scripts/despread_rates.py: gpsiq_despread (seg_len {SEG_LEN}, statistics on) against gpsiq_launch (default variant) of the same blocks, kernel id {gpsiq.kernels_id()}",
             "# config | despread kernel ms | despread without statistics ms | launch ms | stream bytes at the 8 TB/s read roof ms | despread / launch | despread G samples/s | kernel, slots, grid, rows per wave"]
    for name, fs, ss, nb in CONFIGS:
        nsamp = int(round(fs / 10))
        q = gpsiq.quantize_blocks(synth_blocks(nb, 16, seed=1), fs, nsamp)[0]
        ctx.set_descriptors(q)
        stride = 2 * nsamp * ss
        buf = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 3, stream=s)               # warm-up; renders the stream
        launch = min(ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 10, stream=s) for _ in range(5))
        res = []
        for stats in (True, False):
            ctx.despread(0, nb, nsamp, ss, buf.data_ptr(), stride, SEG_LEN, clip=100, stream=s, stats=stats)      # warm-up (buffers)
            res.append(min(ctx.despread(0, nb, nsamp, ss, buf.data_ptr(), stride, SEG_LEN, clip=100, stream=s, stats=stats)[3] for _ in range(5)))
        plan = ctx.despread_last_plan()
        roof = nb * stride / (HBM_PEAK_GBS * 1e9) * 1e3
        lines.append(f"{name} | {res[0]:.3f} | {res[1]:.3f} | {launch:.3f} | {roof:.3f} | {res[0] / launch:.2f} | {nb * nsamp / (res[0] * 1e-3) / 1e9:.1f} | {plan[0]}, {plan[1]}, {plan[2]}, {plan[3]}")
        del buf
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
