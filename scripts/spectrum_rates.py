"""profiles/spectrum_rates.txt: what the spectrum stage costs, and which of its two kernels the planner should take by default
(csrc/gpsiq_spectrum_plan.h, kSpecMfmaDefault).  One span of 26e6 samples of random full-range elements, all segments in one group at
min_shift, every nfft, both hops, both windows:
  int8    both kernels (GPSIQ_SPECTRUM_KERNEL), alternating call by call in the same run
  int16   the generic kernel alone (the matrix kernel serves int8 input)
Every figure is the kernels' device time through kernel_ms, the median of REPEATS calls after two warm-up calls per kernel.  The
yardstick, in the same run: the time the span's bytes take read once at the device's measured copy rate (torch's copy_ of a
contiguous uint8 tensor of 416 MB between events: bytes read plus bytes written over the best of seven).
usage: timeout -k 10 420 python scripts/spectrum_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "spectrum_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    rate = copy_rate()
    lines = [f"# python scripts/spectrum_rates.py: gpsiq_spectrum over one span of {NSAMP} samples, one group, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the two kernels alternate call by call); device-to-device copy rate measured in this run: {rate / 1e9:.0f} GB/s (read + written)",
             "# format | nfft | hop | window | shift | bytes MB | bytes alone ms | generic ms | G samples/s | / bytes | mfma ms | G samples/s | / bytes | default | default is the faster"]
    torch.manual_seed(26)
    src = {SC08: torch.randint(-128, 128, (2 * NSAMP,), dtype=torch.int8, device="cuda"),
           SC16: torch.randint(-32768, 32768, (2 * NSAMP,), dtype=torch.int16, device="cuda")}
    ok = True
    for ss in (SC08, SC16):
        for nfft in (64, 128, 256, 512):
            for hop in (nfft // 2, nfft):
                for window in (0, 1):
                    navg = gpsiq.spectrum_span(NSAMP, nfft, hop, 1)[0]
                    shift = gpsiq.spectrum_min_shift(ss, nfft, window, navg)
                    kernels = ("generic", "mfma") if ss == SC08 else ("generic",)
                    ms = {k: [] for k in kernels}
                    res = {}
                    for rep in range(REPEATS + 2):
                        for k in kernels:
                            os.environ["GPSIQ_SPECTRUM_KERNEL"] = k
                            res[k] = ctx.spectrum(NSAMP, ss, src[ss].data_ptr(), nfft, hop, window, navg, shift)
                            assert ctx.spectrum_last_plan()[0] == k
                            if rep >= 2:
                                ms[k].append(ctx.spectrum_ms)
                    del os.environ["GPSIQ_SPECTRUM_KERNEL"]
                    assert len(kernels) == 1 or res["generic"].tobytes() == res["mfma"].tobytes()
                    ctx.spectrum(NSAMP, ss, src[ss].data_ptr(), nfft, hop, window, navg, shift)
                    default = ctx.spectrum_last_plan()[0]
                    nbytes = 2 * NSAMP * ss
                    alone = nbytes / rate * 1e3
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    cols = []
                    for k in ("generic", "mfma"):
                        cols.append(f"{med[k]:.3f} | {NSAMP / med[k] / 1e6:.1f} | {med[k] / alone:.2f}" if k in med else "- | - | -")
                    fastest = min(med, key=med.get)
                    ok &= default == fastest
                    lines.append(f"int{8 * ss} | {nfft} | {hop} | {'hann' if window else 'rect'} | {shift} | {nbytes / 1e6:.0f} | {alone:.3f} | {cols[0]} | {cols[1]} | {default} | "
                                 f"{'yes' if default == fastest else 'NO'}")
                    print(lines[-1], flush=True)
    lines.append("# the default path is the faster of the two at every row" if ok else "# the default path is NOT the faster at every row: see kSpecMfmaDefault")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3] + lines[-1:]))


if __name__ == "__main__":
    main()
