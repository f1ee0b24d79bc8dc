"""profiles/follow_rates.txt: how fast the follower (gpsiq_follow, include/gpsiq_rows.h, "Follow") gets through a stream -- seconds of
stream followed per second of kernel time for 1, 8 and 32 satellites at 2.6 Msps, int8 and int16.  The stream is two seconds of sixteen
rendered channels (twenty blocks, each a fresh synthetic descriptor set: the loops have something to pull at but nothing to hold,
which costs the same); every satellite starts at sample 0 at the nominal steps, with gpsiq_follow_gains(fs, 0.25, 18, 5).  Per row:
kernel_ms (the minimum of five calls after a warm-up call), the epochs of the longest-running satellite, the launches, and the rate.
No number is promised for this stage: one workgroup per satellite uses a small part of the device and the loop is latency-bound, an
epoch's two barriers and the state thread's scalar code against some ten rows of samples per wave.
usage: timeout -k 10 300 python scripts/follow_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NSAMP, NBLOCKS, MAX_EPOCHS = 2.6e6, 260000, 20, 2200
ROWS = [(name, ss, n) for name, ss in (("int8", SC08), ("int16", SC16)) for n in (1, 8, 32)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "follow_rates.txt")
    ctx = gpsiq.Context(0)
    steps = gpsiq.acquire_steps(FS, 0.0, 250.0)
    cfg = gpsiq.follow_gains(FS, 0.25, 18.0, 5.0)
    seconds = NBLOCKS * NSAMP / FS
    lines = [f"# python scripts/follow_rates.py: gpsiq_follow over {seconds:.1f} s of stream at 2.6 Msps ({NBLOCKS} blocks of {NSAMP} samples, 16 rendered channels), kernel id {gpsiq.kernels_id()}",
             "# row | satellites | kernel ms | epochs of the longest run | launches | seconds of stream per second"]
    q = gpsiq.quantize_blocks(synth_blocks(NBLOCKS, 16, seed=1), FS, NSAMP)[0]
    ctx.set_descriptors(q)
    s = torch.cuda.current_stream().cuda_stream
    for name, ss, nprn in ROWS:
        stride = 2 * NSAMP * ss
        buf = torch.empty(NBLOCKS * stride, dtype=torch.uint8, device="cuda")
        ctx.launch(0, NBLOCKS, NSAMP, ss, buf.data_ptr(), stride, stream=s)
        states = gpsiq.follow_start(list(range(1, nprn + 1)), [0] * nprn, [0] * nprn, *steps)
        best, n = None, None
        for i in range(6):                                              # the first call is the warm-up (buffers)
            _, n, st, ms = ctx.follow(NBLOCKS * NSAMP, ss, buf.data_ptr(), cfg, states, MAX_EPOCHS, stream=s)
            assert all(v == 1 for v in st["status"]), list(st["status"])
            if i and (best is None or ms < best):
                best = ms
        plan = ctx.follow_last_plan()
        lines.append(f"{name} | {nprn} | {best:.3f} | {int(n.max())} | {plan[2]} | {seconds / (best * 1e-3):.1f}")
        del buf
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
