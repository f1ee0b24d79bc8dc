"""profiles/array_rates.txt: what the array stage costs, and where the planner's threshold between the two covariance kernels lies
(csrc/gpsiq_array_plan.h, kArrMfmaMinElem).  Streams of 26e6 samples of random elements per row, at 2, 4 and 8 elements:
  cov int8          array_cov_generic and array_cov_mfma (GPSIQ_ARRAY_KERNEL), alternating call by call in the same run; their
                    numbers are compared at every row
  cov int16         array_cov_generic (there is no int16 matrix kernel)
  combine           array_combine in all four format pairs, weights whose sum |re| + |im| is at most 4096 behind shift 12 (20 from
                    int16 to int8): a gain of at most one
The elements are random over half the format's range, so that the combiner clamps nothing: where it clamps, every workgroup ends in an
atomic add to the call's one counter, and some thousands of adds to one address, about 0.1 ms, hide the kernel (DESIGN.md 8m has the
same for the filters; a first table taken with full-range elements showed exactly that floor).
Every figure is the kernel's device time through kernel_ms, the median of REPEATS calls after two warm-up calls per kernel.  The
yardstick, in the same run: the time the row's bytes alone take -- every element read once, the output (if any) written once -- at
the device's measured copy rate (torch's copy_ of a contiguous uint8 tensor of 416 MB between events: bytes read plus bytes written
over the best of seven).
The last lines name the element counts at which the matrix kernel is the faster: what the threshold must be.
usage: timeout -k 10 420 python scripts/array_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402

NSAMP = 26_000_000
REPEATS = 9
NELEMS = (2, 4, 8)


def copy_rate():
    """bytes per second a device-to-device copy moves, read and written counted"""
    n = 416 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    best = 1e9
    for _ in range(7):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        a.copy_(b)
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return 2 * n / (best * 1e-3)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "array_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    rate = copy_rate()
    lines = [f"# python scripts/array_rates.py: gpsiq_array_cov and gpsiq_array_combine over streams of {NSAMP} samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the two covariance kernels alternate call by call); device-to-device copy rate measured in this run: {rate / 1e9:.0f} GB/s (read + written)",
             "# cov rows:     what | elements | bytes in MB | bytes alone ms | generic ms | GB/s | / bytes | matrix ms | GB/s | / bytes | matrix / generic | default | default is the faster",
             "# combine rows: what | elements | bytes in + out MB | bytes alone ms | ms | GB/s | / bytes"]
    torch.manual_seed(26)
    src = {SC08: [torch.randint(-64, 65, (2 * NSAMP,), dtype=torch.int8, device="cuda") for _ in range(8)],
           SC16: [torch.randint(-16384, 16385, (2 * NSAMP,), dtype=torch.int16, device="cuda") for _ in range(8)]}
    dst = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")
    wins, defaults = {}, {}
    for ss in (SC08, SC16):
        for nelem in NELEMS:
            ptrs = [t.data_ptr() for t in src[ss][:nelem]]
            kernels = ("generic", "mfma") if ss == SC08 else ("generic",)
            ms, cov = {k: [] for k in kernels}, {}
            for rep in range(REPEATS + 2):
                for k in kernels:
                    os.environ["GPSIQ_ARRAY_KERNEL"] = k
                    cov[k], t = ctx.array_cov(ptrs, NSAMP, ss)
                    assert ctx.array_last_plan()[0] == k
                    if rep >= 2:
                        ms[k].append(t)
            del os.environ["GPSIQ_ARRAY_KERNEL"]
            ctx.array_cov(ptrs, NSAMP, ss)
            default = ctx.array_last_plan()[0]
            nbytes = 2 * NSAMP * ss * nelem
            alone = nbytes / rate * 1e3
            med = {k: statistics.median(v) for k, v in ms.items()}
            cols = [f"{med[k]:.3f} | {nbytes / med[k] / 1e6:.0f} | {med[k] / alone:.2f}" if k in med else "- | - | -" for k in ("generic", "mfma")]
            if ss == SC08:
                assert np.array_equal(cov["generic"], cov["mfma"]), "the two kernels gave different numbers"
                fastest = "generic" if med["generic"] <= med["mfma"] else "mfma"
                wins[nelem], defaults[nelem] = fastest == "mfma", default == "mfma"
                tail = f"{med['mfma'] / med['generic']:.2f} | {default} | {'yes' if default == fastest else 'NO'}"
            else:
                tail = f"- | {default} | yes"
            lines.append(f"cov int{8 * ss} | E={nelem} | {nbytes / 1e6:.0f} | {alone:.3f} | {cols[0]} | {cols[1]} | {tail}")
            print(lines[-1], flush=True)
    rng = np.random.default_rng(26)
    for ss in (SC08, SC16):
        for out_ss in (SC08, SC16):
            for nelem in NELEMS:
                ptrs = [t.data_ptr() for t in src[ss][:nelem]]
                lim = 2048 // (2 * (nelem - 1))
                w = rng.integers(-lim, lim + 1, size=(nelem, 2)).astype(np.int16)
                w[0] = (2048, 0)                                      # sum |re| + |im| <= 4096: a gain of at most one behind the shift
                shift = 12 + 8 * (ss - out_ss if ss > out_ss else 0)
                runs = [ctx.array_combine(ptrs, NSAMP, ss, w, shift, out_ss, dst.data_ptr()) for _ in range(REPEATS + 2)][2:]
                assert all(c == 0 for c, _ in runs), "an element was clamped: the counter's atomics would be timed"
                ts = [t for _, t in runs]
                nbytes = 2 * NSAMP * (ss * nelem + out_ss)
                alone = nbytes / rate * 1e3
                med = statistics.median(ts)
                lines.append(f"combine int{8 * ss} -> int{8 * out_ss} | E={nelem} | {nbytes / 1e6:.0f} | {alone:.3f} | {med:.3f} | {nbytes / med / 1e6:.0f} | {med / alone:.2f}")
                print(lines[-1], flush=True)
    faster = [e for e in NELEMS if wins[e]]
    ok = all(defaults[e] == wins[e] for e in NELEMS)
    lines.append(f"# int8 covariance: the matrix kernel is the faster at {', '.join(str(e) for e in faster)} elements" if faster else
                 "# int8 covariance: the matrix kernel is the faster at no measured element count: the generic kernel is the default, GPSIQ_ARRAY_KERNEL=mfma reaches the other")
    lines.append("# the planner's defaults are those element counts" if ok else "# the planner's defaults are NOT those element counts: move kArrMfmaMinElem")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2] + lines[-2:]))


if __name__ == "__main__":
    main()
