"""profiles/stap_rates.txt: what the space-time array stage costs, and where the planner's threshold between the two covariance
kernels lies (csrc/gpsiq_stap_plan.h, kStapMfmaMinRows).  Streams of 26e6 samples of random elements per row, at
(elements, taps) = (2, 1), (2, 2) (the rows below one full group), (2, 4), (4, 2), (4, 4), (4, 8), (8, 4), with heads:
  cov int8          stap_cov_generic and stap_cov_mfma<G> (GPSIQ_STAP_KERNEL), alternating call by call in the same run; their
                    numbers are compared at every row
  cov int16         stap_cov_generic (there is no int16 matrix kernel)
  combine           stap_combine in all four format pairs, weights whose sum |re| + |im| is at most 4096 behind shift 12 (20 from
                    int16 to int8): a gain of at most one
  array ...         gpsiq_array_cov (its default kernel) and gpsiq_array_combine at the same element count: the yardstick for one tap
The elements are random over half the format's range, so that the combiner clamps nothing (asserted): where it clamps, every
workgroup ends in an atomic add to the call's one counter (scripts/array_rates.py has the reason).
Every figure is the kernel's device time through kernel_ms, the median of REPEATS calls after two warm-up calls per kernel.  The
yardstick, in the same run: the time the row's bytes alone take -- every element read once, the output (if any) written once -- at
the device's measured copy rate (torch's copy_ of a contiguous uint8 tensor of 416 MB between events: bytes read plus bytes written
over the best of seven).
The last lines name the shapes at which the matrix kernel is the faster: what the threshold must allow.
usage: timeout -k 10 540 python scripts/stap_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from array_rates import copy_rate  # noqa: E402

NSAMP = 26_000_000
REPEATS = 7
SHAPES = ((2, 1), (2, 2), (2, 4), (4, 2), (4, 4), (4, 8), (8, 4))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stap_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    rate = copy_rate()
    lines = [f"# python scripts/stap_rates.py: gpsiq_stap_cov and gpsiq_stap_combine over streams of {NSAMP} samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the two covariance kernels alternate call by call); device-to-device copy rate measured in this run: {rate / 1e9:.0f} GB/s (read + written)",
             "# cov rows:     what | elements x taps | bytes in MB | bytes alone ms | generic ms | / bytes | matrix ms | / bytes | matrix / generic | default | default is the faster | array_cov at E ms",
             "# combine rows: what | elements x taps | bytes in + out MB | bytes alone ms | ms | GB/s | / bytes | array_combine at E ms"]
    torch.manual_seed(26)
    src = {SC08: [torch.randint(-64, 65, (2 * NSAMP,), dtype=torch.int8, device="cuda") for _ in range(8)],
           SC16: [torch.randint(-16384, 16385, (2 * NSAMP,), dtype=torch.int16, device="cuda") for _ in range(8)]}
    heads = {SC08: [torch.randint(-64, 65, (16,), dtype=torch.int8, device="cuda") for _ in range(8)],
             SC16: [torch.randint(-16384, 16385, (16,), dtype=torch.int16, device="cuda") for _ in range(8)]}
    dst = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")
    wins, defaults = {}, {}
    for ss in (SC08, SC16):
        for nelem, ntaps in SHAPES:
            ptrs = [t.data_ptr() for t in src[ss][:nelem]]
            hptrs = [t.data_ptr() for t in heads[ss][:nelem]]
            kernels = ("generic", "mfma") if ss == SC08 else ("generic",)
            ms, cov = {k: [] for k in kernels}, {}
            for rep in range(REPEATS + 2):
                for k in kernels:
                    os.environ["GPSIQ_STAP_KERNEL"] = k
                    cov[k], t = ctx.stap_cov(ptrs, NSAMP, ss, ntaps, heads=hptrs)
                    assert ctx.stap_last_plan()[0] == k
                    if rep >= 2:
                        ms[k].append(t)
            del os.environ["GPSIQ_STAP_KERNEL"]
            ctx.stap_cov(ptrs, NSAMP, ss, ntaps, heads=hptrs)
            default = ctx.stap_last_plan()[0]
            arr = statistics.median([ctx.array_cov(ptrs, NSAMP, ss)[1] for _ in range(REPEATS + 2)][2:])
            nbytes = 2 * NSAMP * ss * nelem
            alone = nbytes / rate * 1e3
            med = {k: statistics.median(v) for k, v in ms.items()}
            cols = [f"{med[k]:.3f} | {med[k] / alone:.2f}" if k in med else "- | -" for k in ("generic", "mfma")]
            if ss == SC08:
                assert np.array_equal(cov["generic"], cov["mfma"]), "the two kernels gave different numbers"
                fastest = "generic" if med["generic"] <= med["mfma"] else "mfma"
                wins[(nelem, ntaps)], defaults[(nelem, ntaps)] = fastest == "mfma", default == "mfma"
                tail = f"{med['mfma'] / med['generic']:.2f} | {default} | {'yes' if default == fastest else 'NO'}"
            else:
                tail = f"- | {default} | yes"
            lines.append(f"cov int{8 * ss} | {nelem} x {ntaps} | {nbytes / 1e6:.0f} | {alone:.3f} | {cols[0]} | {cols[1]} | {tail} | {arr:.3f}")
            print(lines[-1], flush=True)
    rng = np.random.default_rng(26)
    for ss in (SC08, SC16):
        for out_ss in (SC08, SC16):
            for nelem, ntaps in SHAPES:
                ptrs = [t.data_ptr() for t in src[ss][:nelem]]
                hptrs = [t.data_ptr() for t in heads[ss][:nelem]]
                rows = nelem * ntaps
                lim = 2048 // (2 * (rows - 1))
                w = rng.integers(-lim, lim + 1, size=(nelem, ntaps, 2)).astype(np.int16)
                w[0, 0] = (2048, 0)                                   # sum |re| + |im| <= 4096: a gain of at most one behind the shift
                shift = 12 + 8 * (ss - out_ss if ss > out_ss else 0)
                runs = [ctx.stap_combine(ptrs, NSAMP, ss, w, shift, out_ss, dst.data_ptr(), heads=hptrs) for _ in range(REPEATS + 2)][2:]
                assert all(c == 0 for c, _ in runs), "an element was clamped: the counter's atomics would be timed"
                aruns = [ctx.array_combine(ptrs, NSAMP, ss, w[:, 0], shift, out_ss, dst.data_ptr()) for _ in range(REPEATS + 2)][2:]
                assert all(c == 0 for c, _ in aruns)
                nbytes = 2 * NSAMP * (ss * nelem + out_ss)
                alone = nbytes / rate * 1e3
                med, amed = statistics.median([t for _, t in runs]), statistics.median([t for _, t in aruns])
                lines.append(f"combine int{8 * ss} -> int{8 * out_ss} | {nelem} x {ntaps} | {nbytes / 1e6:.0f} | {alone:.3f} | {med:.3f} | {nbytes / med / 1e6:.0f} | "
                             f"{med / alone:.2f} | {amed:.3f}")
                print(lines[-1], flush=True)
    faster = [s for s in SHAPES if wins[s]]
    ok = all(defaults[s] == wins[s] for s in SHAPES)
    lines.append("# int8 covariance: the matrix kernel is the faster at " + ", ".join(f"{e} x {t}" for e, t in faster) if faster else
                 "# int8 covariance: the matrix kernel is the faster at no measured shape: GPSIQ_STAP_KERNEL=mfma reaches it")
    lines.append("# the planner's defaults are those shapes" if ok else "# the planner's defaults are NOT those shapes: move kStapMfmaMinRows")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2] + lines[-2:]))


if __name__ == "__main__":
    main()
