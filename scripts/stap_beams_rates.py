"""profiles/stap_beams_rates.txt: what gpsiq_stap_beams costs, and where the planner's threshold between its two kernels lies
(csrc/gpsiq_stap_beams_plan.h, beams_mfma_min_rows).  Streams of 26e6 samples of random elements per row, at
(elements, taps) = (2, 1), (2, 4), (4, 4), (4, 8), (8, 4) with heads, 1, 2, 4 and 8 beams, int8 -> int8 and int16 -> int16:
  generic     stap_beams_generic  }  GPSIQ_STAP_BEAMS_KERNEL, alternating call by call in the same run; their bytes are compared
  matrix      stap_beams_mfma     }  at every row
  combine     nbeams calls of the existing gpsiq_stap_combine on the same inputs, their kernel times added: what a receiver pays
              today, and the comparison that matters
Weights whose sum |re| + |im| is at most 4096 per beam behind shift 12: a gain of at most one.  The elements are random over half the
format's range, so that nothing is clamped (asserted): where a beam clamps, every workgroup ends in an atomic add to its counter.
Every figure is the kernel's device time through kernel_ms, the median of REPEATS calls after two warm-up calls per kernel, with the
least and the greatest of them in the last two columns: a ratio within that spread of 1 decides nothing.  The
yardstick, in the same run: the time the row's bytes alone take -- every element read once, every beam written once -- at the
device's measured copy rate (scripts/array_rates.py, copy_rate).
The last lines name the rows at which the matrix kernel is the faster of the two: what the thresholds must allow.
usage: timeout -k 10 540 python scripts/stap_beams_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
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
SHAPES = ((2, 1), (2, 4), (4, 4), (4, 8), (8, 4))
BEAMS = (1, 2, 4, 8)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stap_beams_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    rate = copy_rate()
    lines = [f"# python scripts/stap_beams_rates.py: gpsiq_stap_beams over streams of {NSAMP} samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the kernels alternate call by call); device-to-device copy rate measured in this run: {rate / 1e9:.0f} GB/s (read + written)",
             "# formats | elements x taps | beams | bytes in + out MB | bytes alone ms | generic ms | / bytes | matrix ms | / bytes | matrix / generic | "
             "beams x stap_combine ms | matrix / that | generic / that | default | default is the faster | generic min .. max ms | matrix min .. max ms"]
    torch.manual_seed(27)
    src = {SC08: [torch.randint(-64, 65, (2 * NSAMP,), dtype=torch.int8, device="cuda") for _ in range(8)],
           SC16: [torch.randint(-16384, 16385, (2 * NSAMP,), dtype=torch.int16, device="cuda") for _ in range(8)]}
    heads = {SC08: [torch.randint(-64, 65, (16,), dtype=torch.int8, device="cuda") for _ in range(8)],
             SC16: [torch.randint(-16384, 16385, (16,), dtype=torch.int16, device="cuda") for _ in range(8)]}
    dst = [torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda") for _ in range(8)]
    check = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(27)
    wins, defaults = {}, {}
    for ss in (SC08, SC16):
        for nelem, ntaps in SHAPES:
            ptrs = [t.data_ptr() for t in src[ss][:nelem]]
            hptrs = [t.data_ptr() for t in heads[ss][:nelem]]
            rows = nelem * ntaps
            for nbeams in BEAMS:
                lim = 2048 // (2 * (rows - 1))
                w = rng.integers(-lim, lim + 1, size=(nbeams, nelem, ntaps, 2)).astype(np.int16)
                w[:, 0, 0] = (2048, 0)                                # sum |re| + |im| <= 4096 per beam
                dptrs = [t.data_ptr() for t in dst[:nbeams]]
                ms = {"generic": [], "mfma": []}
                for rep in range(REPEATS + 2):
                    for k in ms:
                        os.environ["GPSIQ_STAP_BEAMS_KERNEL"] = k
                        c, t = ctx.stap_beams(ptrs, NSAMP, ss, w, 12, ss, dptrs, heads=hptrs)
                        assert ctx.stap_beams_last_plan()[0] == k and not c.any(), "an element was clamped: the counters' atomics would be timed"
                        if rep >= 2:
                            ms[k].append(t)
                        if rep == 0 and k == "generic":
                            check.copy_(dst[nbeams - 1])
                        if rep == 0 and k == "mfma":
                            assert torch.equal(check[:2 * NSAMP * ss], dst[nbeams - 1][:2 * NSAMP * ss]), "the two kernels wrote different bytes"
                del os.environ["GPSIQ_STAP_BEAMS_KERNEL"]
                ctx.stap_beams(ptrs, NSAMP, ss, w, 12, ss, dptrs, heads=hptrs)
                default = ctx.stap_beams_last_plan()[0]
                single = []
                for rep in range(REPEATS + 2):
                    total = 0.0
                    for b in range(nbeams):
                        c, t = ctx.stap_combine(ptrs, NSAMP, ss, w[b], 12, ss, dptrs[b], heads=hptrs)
                        assert c == 0
                        total += t
                    if rep >= 2:
                        single.append(total)
                nbytes = 2 * NSAMP * ss * (nelem + nbeams)
                alone = nbytes / rate * 1e3
                g, m, s = statistics.median(ms["generic"]), statistics.median(ms["mfma"]), statistics.median(single)
                fastest = "generic" if g <= m else "mfma"
                wins[(ss, nelem, ntaps, nbeams)], defaults[(ss, nelem, ntaps, nbeams)] = fastest == "mfma", default == "mfma"
                lines.append(f"int{8 * ss} -> int{8 * ss} | {nelem} x {ntaps} | {nbeams} | {nbytes / 1e6:.0f} | {alone:.3f} | {g:.3f} | {g / alone:.2f} | {m:.3f} | "
                             f"{m / alone:.2f} | {m / g:.2f} | {s:.3f} | {m / s:.2f} | {g / s:.2f} | {default} | {'yes' if default == fastest else 'NO'} | "
                             f"{min(ms['generic']):.3f} .. {max(ms['generic']):.3f} | {min(ms['mfma']):.3f} .. {max(ms['mfma']):.3f}")
                print(lines[-1], flush=True)
    faster = [k for k in wins if wins[k]]
    lines.append("# the matrix kernel is the faster at " + (", ".join(f"int{8 * ss} {e} x {t} x {b}" for ss, e, t, b in faster) if faster else "no measured row"))
    off = [k for k in wins if defaults[k] != wins[k]]
    lines.append("# the planner's default is the faster kernel at every measured row" if not off else
                 "# the planner's default is not the faster kernel at " + ", ".join(f"int{8 * ss} {e} x {t} x {b}" for ss, e, t, b in off) +
                 ": beams_mfma_min_rows asks for every measured row of that size or larger")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:2] + lines[-2:]))


if __name__ == "__main__":
    main()
