"""profiles/agc_rates.txt: what the gain control stage costs.  One span of 2^20, 2^24 and 2^27 samples of random full-range elements, int8
to int8 and int16 to int16, window 1024, navg 16, with the blanker off and on (a threshold only the most negative value exceeds, a hold of
64 samples): the device time of each of the three launches (agc_measure, agc_gains, agc_apply: gpsiq_agc_last_ms), of the three together
(kernel_ms) and the wall time of the call, each the median of REPEATS calls after two warm-up calls.  Bytes moved: the span twice (both
element-wise passes read it) plus what dst receives.  The yardstick, in the same run: gpsiq_pack of the same span to 4 bits (2 bits for
int16 would halve its writes again), the project's other pure stream pass, by its own kernel_ms, and the bytes it moves.
usage: timeout -k 10 420 python scripts/agc_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402

SPANS = (1 << 20, 1 << 24, 1 << 27)
REPEATS = 9


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "agc_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    torch.manual_seed(27)
    most = max(SPANS)
    x = {SC08: torch.randint(-128, 128, (2 * most,), dtype=torch.int8, device="cuda"),
         SC16: torch.randint(-32768, 32768, (2 * most,), dtype=torch.int16, device="cuda")}
    work = torch.empty(4 * most, dtype=torch.uint8, device="cuda")
    lines = [f"# python scripts/agc_rates.py: gpsiq_agc over one span, window 1024, navg 16, kernel id {gpsiq.kernels_id()}",
             f"# device ms, median of {REPEATS} calls; bytes moved: the span twice and the destination once; pack: gpsiq_pack of the same span to 4 bits, in this run",
             "# shape | samples | blanker | measure ms | gains ms | apply ms | three launches ms | call wall ms | MB moved | GB/s | pack ms | pack MB | pack GB/s | launches / pack"]
    for ss in (SC08, SC16):
        for nsamp in SPANS:
            pack_ms = []
            for rep in range(REPEATS + 2):
                _, t = ctx.pack(1, nsamp, ss, x[ss].data_ptr(), 2 * nsamp * ss, 4, work.data_ptr(), nsamp)
                if rep >= 2:
                    pack_ms.append(t)
            pack = statistics.median(pack_ms)
            pack_mb = (2 * nsamp * ss + nsamp) / 1e6
            for blanker in (False, True):
                cfg = gpsiq.AgcCfg(window=1024, navg=16, target_q8=256 * (40 if ss == SC08 else 9000), mult0=65536,
                                   blank_thresh=(127 if ss == SC08 else 32767) if blanker else 0, blank_hold=64 if blanker else 0, qmax=127 if ss == SC08 else 32767)
                parts, whole, wall = [], [], []
                for rep in range(REPEATS + 2):
                    st = gpsiq.AgcState()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    clipped, blanked, mults, ms = ctx.agc(nsamp, ss, x[ss].data_ptr(), cfg, ss, work.data_ptr(), state=st)
                    t1 = time.perf_counter()
                    if rep >= 2:
                        parts.append(ctx.agc_last_ms())
                        whole.append(ms)
                        wall.append(1e3 * (t1 - t0))
                assert (blanked > 0) == blanker and len(mults) == nsamp // 1024
                m = [statistics.median(p[i] for p in parts) for i in range(3)]
                w = statistics.median(whole)
                moved = (2 * 2 * nsamp * ss + 2 * nsamp * ss + (nsamp // 8 * 2 if blanker else 0)) / 1e6
                lines.append(f"int{8 * ss} to int{8 * ss} | {nsamp} | {'on' if blanker else 'off'} | {m[0]:.4f} | {m[1]:.4f} | {m[2]:.4f} | {w:.4f} | "
                             f"{statistics.median(wall):.4f} | {moved:.1f} | {moved / w:.0f} | {pack:.4f} | {pack_mb:.1f} | {pack_mb / pack:.0f} | {w / pack:.2f}")
                print(lines[-1], flush=True)
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
