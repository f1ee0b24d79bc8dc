"""profiles/acquire_rates.txt: what the blind search (gpsiq_acquire, include/gpsiq_rows.h, "Acquisition") costs at the workload's own
shape -- one 2.6 Msps block, 32 satellites, 41 bins of 500 Hz, 2 600 shifts (one code period), ncoh 2 560, hop 2 600, with 1 and with
10 dwells, int8 and the int16 row.  Per row: kernel_ms (the minimum of five calls after a warm-up call) of stage one (acquire_wipe), of
stage two (acquire_mfma + acquire_peaks) and of the generic kernel (+ acquire_peaks), the ratio generic / matrix path, the integer
multiply-adds per second of stage two -- those the contract's sums need in digit form (satellites x bins x shifts x ncoh x dwells x 2
x digits) and those the MFMAs issue (16 384 each, padding included) -- against the int8 matrix peak of MI355X_MICROARCH.md (2x the
2.5 PFLOP/s of bf16: 2.5e15 multiply-adds a second), and, timed in the same run, the gpsiq_launch that rendered the block.  Both
kernels' peaks are compared byte for byte before anything is written.
usage: timeout -k 10 600 python scripts/acquire_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

INT8_PEAK_MACS = 2.5e15
FS, NSAMP, NPRN, NDOPP, NSHIFT, NCOH, HOP = 2.6e6, 260000, 32, 41, 2600, 2560, 2600
ROWS = [("int8, 1 dwell", SC08, 1), ("int8, 10 dwells", SC08, 10), ("int16, 1 dwell", SC16, 1), ("int16, 10 dwells", SC16, 10)]


def timed(ctx, kernel, ss, ptr, steps, nn, s):
    os.environ["GPSIQ_ACQUIRE_KERNEL"] = kernel
    best, peaks = None, None
    for i in range(6):                                                  # the first call is the warm-up (buffers)
        peaks, _, _, ms = ctx.acquire(NSAMP, ss, ptr, list(range(1, NPRN + 1)), *steps, NDOPP, NSHIFT, NCOH, nn, HOP, stream=s, power=False)
        plan = ctx.acquire_last_plan()
        assert plan[0] == kernel, plan
        if i and (best is None or plan[4] + plan[5] < best[0] + best[1]):
            best = (plan[4], plan[5], plan)
    del os.environ["GPSIQ_ACQUIRE_KERNEL"]
    return best, peaks


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "acquire_rates.txt")
    ctx = gpsiq.Context(0)
    steps = gpsiq.acquire_steps(FS, -10000.0, 500.0)
    lines = [f"# python scripts/acquire_rates.py: gpsiq_acquire of one {NSAMP}-sample block at 2.6 Msps, {NPRN} satellites x {NDOPP} bins x {NSHIFT} shifts, ncoh {NCOH}, hop {HOP}, kernel id {gpsiq.kernels_id()}",
             "# row | wipe ms | mfma + peaks ms | matrix path ms | generic + peaks ms | generic / matrix path | needed digit MAC/s of stage two, share of the int8 peak | issued MAC/s, share | launch of the block ms | workgroups, k-steps, plane bytes"]
    for name, ss, nn in ROWS:
        q = gpsiq.quantize_blocks(synth_blocks(1, 16, seed=1), FS, NSAMP)[0]
        ctx.set_descriptors(q)
        stride = 2 * NSAMP * ss
        buf = torch.empty(stride, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        ctx.time_launches(0, 1, NSAMP, ss, buf.data_ptr(), stride, 3, stream=s)                    # warm-up; renders the block
        launch = min(ctx.time_launches(0, 1, NSAMP, ss, buf.data_ptr(), stride, 10, stream=s) for _ in range(5))
        fast, pf = timed(ctx, "mfma", ss, buf.data_ptr(), steps, nn, s)
        slow, pg = timed(ctx, "generic", ss, buf.data_ptr(), steps, nn, s)
        assert pf.tobytes() == pg.tobytes(), "the two kernels disagree"
        digits = 3 if ss == SC08 else 4
        needed = NPRN * NDOPP * NSHIFT * NCOH * nn * 2 * digits
        plan = fast[2]
        waves = NPRN * ((NSHIFT + 255) // 256) * ((NDOPP + 1) // 2)      # one per (satellite, 256 shifts, row tile)
        issued = waves * 16 * plan[3] * nn * 16384                   # x tiles per wave x k-steps x dwells x multiply-adds of one MFMA
        both, gen = fast[0] + fast[1], slow[0] + slow[1]
        lines.append(f"{name} | {fast[0]:.3f} | {fast[1]:.3f} | {both:.3f} | {gen:.3f} | {gen / both:.2f} | {needed / (fast[1] * 1e-3):.3e}, {needed / (fast[1] * 1e-3) / INT8_PEAK_MACS:.3f} | "
                     f"{issued / (fast[1] * 1e-3):.3e}, {issued / (fast[1] * 1e-3) / INT8_PEAK_MACS:.3f} | {launch:.3f} | {plan[2]}, {plan[3]}, {plan[1]}")
        del buf
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
