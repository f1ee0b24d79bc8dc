"""profiles/cfilter_rates.txt: what the complex filter costs, and where the planner's thresholds between its kernels lie
(csrc/gpsiq_cfilter_plan.h, kCfiltMfmaMinTaps8 and kCfiltMfmaMinTaps16).  One span of 26e6 input samples of random elements of half
the format's range per row (a notch passes the band at a gain of one: with full-range elements one element in some hundreds is
clamped, every workgroup then ends in an atomic add to the one counter, and those 25 000 adds in a row, about 0.3 ms, hide both
kernels), filtered with gpsiq_notch_design's taps (one line at +300 kHz, shift 12) at 5, 9, 17, 33, 65, 129 and 257 taps, decimated by 1
and by 4:
  int8 -> int8      cfilter_generic and filter_mfma with complex planes (GPSIQ_CFILTER_KERNEL), alternating call by call in the same
                    run, and gpsiq_filter (real taps of the same length, its own default kernel) on the same span beside them
  int16 -> int16    cfilter_generic and cfilter_mfma16, alternating likewise
Every figure is the kernel's device time through kernel_ms, the median of REPEATS calls after two warm-up calls per kernel; the two
kernels' bytes are compared at every row.  The yardstick, in the same run: the time the row's bytes alone take -- input read once,
output written once -- at the device's measured copy rate (torch's copy_ of a contiguous uint8 tensor of 416 MB between events: bytes
read plus bytes written over the best of seven).
The last lines name, per input format, the smallest measured ntaps from which the matrix kernel is the faster at every larger
measured row (both decimations): what the threshold must be.
usage: timeout -k 10 420 python scripts/cfilter_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402

NSAMP = 26_000_000
FS = 10.4e6
REPEATS = 9
NTAPS = (5, 9, 17, 33, 65, 129, 257)
MATRIX = {SC08: "mfma", SC16: "mfma16"}


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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cfilter_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    rate = copy_rate()
    lines = [f"# python scripts/cfilter_rates.py: gpsiq_cfilter over one span of {NSAMP} input samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the kernels alternate call by call); device-to-device copy rate measured in this run: {rate / 1e9:.0f} GB/s (read + written)",
             "# formats | taps | decim | bytes in + out MB | bytes alone ms | generic ms | G samples/s | / bytes | matrix ms | G samples/s | / bytes | matrix / generic | gpsiq_filter ms (real taps, its default kernel) | default | default is the faster"]
    torch.manual_seed(26)
    src = {SC08: torch.randint(-64, 65, (2 * NSAMP,), dtype=torch.int8, device="cuda"),
           SC16: torch.randint(-16384, 16385, (2 * NSAMP,), dtype=torch.int16, device="cuda")}
    dst = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")
    other = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")
    wins = {SC08: {}, SC16: {}}                                       # format -> ntaps -> the matrix kernel is the faster at both decimations
    defaults = {SC08: {}, SC16: {}}                                   # format -> ntaps -> the planner's default is the matrix kernel
    for ss in (SC08, SC16):
        for ntaps in NTAPS:
            taps = gpsiq.notch_design(FS, [300e3], FS / 8, ntaps, 12)
            real = gpsiq.filter_design(FS, 1.2e6, ntaps, 14)
            for decim in (1, 4):
                ms = {"generic": [], "mfma": [], "filter": []}
                for rep in range(REPEATS + 2):
                    for k in ("generic", "mfma"):
                        os.environ["GPSIQ_CFILTER_KERNEL"] = k
                        nout, clipped, t = ctx.cfilter(NSAMP, ss, src[ss].data_ptr(), taps, 12, decim, 0, ss, dst.data_ptr())
                        assert clipped == 0 and ctx.cfilter_last_plan()[0] == ("generic" if k == "generic" else MATRIX[ss])
                        if rep >= 2:
                            ms[k].append(t)
                    if ss == SC08:
                        t = ctx.filter(NSAMP, ss, src[ss].data_ptr(), real, 14, decim, 0, ss, other.data_ptr())[2]
                        if rep >= 2:
                            ms["filter"].append(t)
                os.environ["GPSIQ_CFILTER_KERNEL"] = "generic"             # (the matrix kernel wrote dst last) the bytes at the size timed
                ctx.cfilter(NSAMP, ss, src[ss].data_ptr(), taps, 12, decim, 0, ss, other.data_ptr())
                assert torch.equal(dst[:2 * nout * ss], other[:2 * nout * ss]), "the two kernels wrote different bytes"
                del os.environ["GPSIQ_CFILTER_KERNEL"]
                ctx.cfilter(NSAMP, ss, src[ss].data_ptr(), taps, 12, decim, 0, ss, dst.data_ptr())
                default = ctx.cfilter_last_plan()[0]
                nbytes = 2 * NSAMP * ss + 2 * nout * ss
                alone = nbytes / rate * 1e3
                med = {k: statistics.median(v) for k, v in ms.items() if v}
                cols = [f"{med[k]:.3f} | {NSAMP / med[k] / 1e6:.1f} | {med[k] / alone:.2f}" for k in ("generic", "mfma")]
                fastest = "generic" if med["generic"] <= med["mfma"] else MATRIX[ss]
                wins[ss][ntaps] = wins[ss].get(ntaps, True) and fastest != "generic"
                defaults[ss][ntaps] = default != "generic"
                filt = f"{med['filter']:.3f}" if "filter" in med else "-"
                lines.append(f"int{8 * ss} -> int{8 * ss} | {ntaps} | {decim} | {nbytes / 1e6:.0f} | {alone:.3f} | {cols[0]} | {cols[1]} | {med['mfma'] / med['generic']:.2f} | "
                             f"{filt} | {default} | {'yes' if default == fastest else 'NO'}")
                print(lines[-1], flush=True)
    ok = True
    for ss in (SC08, SC16):
        least = None
        for ntaps in reversed(NTAPS):
            if not wins[ss][ntaps]:
                break
            least = ntaps
        ok &= all(defaults[ss][ntaps] == (least is not None and ntaps >= least) for ntaps in NTAPS)
        lines.append(f"# int{8 * ss} input: the matrix kernel is the faster at every measured row from {least} taps on" if least else
                     f"# int{8 * ss} input: the matrix kernel is not the faster from any measured ntaps on: the generic kernel is the default")
    lines.append("# the planner's defaults are those thresholds (a row marked NO below its format's threshold is one the rule leaves to the generic kernel)" if ok else
                 "# the planner's defaults are NOT those thresholds: move kCfiltMfmaMinTaps8 / kCfiltMfmaMinTaps16")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3] + lines[-3:]))


if __name__ == "__main__":
    main()
