"""profiles/resample_rates.txt: what the resampler stage costs, and which of its two kernels the planner should take by default
(csrc/gpsiq_resample_plan.h, kRsDefaultKernel).  One span of 26e6 input samples of random full-range elements, designed taps
(gpsiq_resample_design, bandwidth 0.8, shift 14):
  int8 to int8 and int16 to int16 at 2.6 to 2.048 Msps, 128 phases of 16 taps, without and with interpolation between the phases
  int8 at a clock offset of 20 ppm (step 2^32 (1 + 20e-6)): every lane of a wave reads the same row of the table
  int8 at eight input samples an output (step 2^35) and at eight outputs an input sample (step 2^29)
  int8 at 2.6 to 2.048 Msps with 64 phases of 64 taps
Both kernels (GPSIQ_RESAMPLE_KERNEL) alternate call by call in the same run; every figure is the kernel's device time through
kernel_ms, the median of REPEATS calls after two warm-up calls per kernel, and the two kernels' bytes and counts are compared.  Bytes
moved: what the span holds plus what dst receives.  The yardstick, in the same run and not our code: a device-to-device
hipMemcpyAsync (torch's copy_ of a contiguous uint8 tensor, between events) that moves the same byte count, half of it read and
half written; median of REPEATS.
usage: timeout -k 10 420 python scripts/resample_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402

NSAMP = 26_000_000
REPEATS = 9
ONE = 1 << 32


def copy_ms(nbytes):
    """milliseconds a device-to-device copy of nbytes takes (nbytes read, nbytes written)"""
    a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ms = []
    for rep in range(REPEATS + 2):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        a.copy_(b)
        t1.record()
        t1.synchronize()
        if rep >= 2:
            ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    torch.manual_seed(26)
    x = {SC08: torch.randint(-128, 128, (2 * NSAMP,), dtype=torch.int8, device="cuda"),
         SC16: torch.randint(-32768, 32768, (2 * NSAMP,), dtype=torch.int16, device="cuda")}
    down = gpsiq.resample_step(2.6e6, 2.048e6)
    # (name, sample size in and out, step, log2 phases, taps, interp)
    shapes = [("int8 2.6 to 2.048 Msps, 128 x 16", SC08, down, 7, 16, 0), ("int8 2.6 to 2.048 Msps, 128 x 16, interp", SC08, down, 7, 16, 1),
              ("int16 2.6 to 2.048 Msps, 128 x 16", SC16, down, 7, 16, 0), ("int16 2.6 to 2.048 Msps, 128 x 16, interp", SC16, down, 7, 16, 1),
              ("int8 1 + 20e-6, 128 x 16, interp", SC08, gpsiq.resample_step(2.6e6, 2.6e6, -20000.0), 7, 16, 1),
              ("int8 8 down, 128 x 16, interp", SC08, 1 << 35, 7, 16, 1), ("int8 8 up, 128 x 16, interp", SC08, 1 << 29, 7, 16, 1),
              ("int8 2.6 to 2.048 Msps, 64 x 64, interp", SC08, down, 6, 64, 1)]
    most = gpsiq.resample_span(NSAMP, 0, 1 << 29)[0]
    work = torch.empty(2 * most * 2, dtype=torch.uint8, device="cuda")
    lines = [f"# python scripts/resample_rates.py: gpsiq_resample over one span of {NSAMP} input samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the two kernels alternate call by call); copy: a device-to-device hipMemcpyAsync of the same byte count, measured in this run",
             "# shape | outputs | bytes moved MB | copy ms | generic ms | GB/s | / copy | rows ms | GB/s | / copy | rows / generic | default | default is the faster"]
    ok = True
    for name, ss, step, L, ntaps, interp in shapes:
        taps = gpsiq.resample_design(step, 0.8, L, ntaps, 14)
        nout = gpsiq.resample_span(NSAMP, 0, step)[0]
        moved = 2 * NSAMP * ss + 2 * nout * ss
        ms = {"generic": [], "rows": []}
        res = {}
        for rep in range(REPEATS + 2):
            for k in ms:
                os.environ["GPSIQ_RESAMPLE_KERNEL"] = k
                n, nxt, clipped, t = ctx.resample(NSAMP, ss, x[ss].data_ptr(), taps, L, 14, interp, step, 0, ss, work.data_ptr())
                assert ctx.resample_last_plan()[0] == k and n == nout
                if rep == 0:
                    res[k] = (clipped, nxt, work[:2 * nout * ss].clone())
                if rep >= 2:
                    ms[k].append(t)
        del os.environ["GPSIQ_RESAMPLE_KERNEL"]
        assert res["generic"][:2] == res["rows"][:2] and torch.equal(res["generic"][2], res["rows"][2]), name
        res.clear()
        ctx.resample(NSAMP, ss, x[ss].data_ptr(), taps, L, 14, interp, step, 0, ss, work.data_ptr())
        default = ctx.resample_last_plan()[0]
        copy = copy_ms(moved // 2)
        med = {k: statistics.median(v) for k, v in ms.items()}
        fastest = min(med, key=med.get)
        ok &= default == fastest
        cols = [f"{med[k]:.3f} | {moved / med[k] / 1e6:.0f} | {med[k] / copy:.2f}" for k in ("generic", "rows")]
        lines.append(f"{name} | {nout} | {moved / 1e6:.0f} | {copy:.3f} | {cols[0]} | {cols[1]} | {med['rows'] / med['generic']:.3f} | {default} | {'yes' if default == fastest else 'NO'}")
        print(lines[-1], flush=True)
    lines.append("# the default path is the faster of the two at every row" if ok else "# the default path is NOT the faster at every row: see kRsDefaultKernel")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3] + lines[-1:]))


if __name__ == "__main__":
    main()
