"""profiles/mix_rates.txt: what the mix stage costs, and which of its two kernels the planner should take by default
(csrc/gpsiq_mix_plan.h, kMixRowsDefault).  One span of 64e6 samples of random full-range elements, four shapes:
  in place, int8      a stream term on dst itself plus one tone
  in place, int16     the same in int16
  repeater, int16     a stream term, the same stream rotated and delayed by 701 samples, two tones (one swept, one gated), into another buffer
  eight terms, int8   three stream terms (int8, int16, int8 delayed by an odd count), two rotated ones, three tones, into another buffer
Both kernels (GPSIQ_MIX_KERNEL) alternate call by call in the same run; every figure is the kernel's device time through kernel_ms,
the median of REPEATS calls after two warm-up calls per kernel, and the two kernels' bytes and counts are compared.  Bytes moved: what
the terms read plus what dst receives.  The yardstick, in the same run and not our code: a device-to-device hipMemcpyAsync (torch's
copy_ of a contiguous uint8 tensor, between events) that moves the same byte count, half of it read and half written; median of
REPEATS.
usage: timeout -k 10 420 python scripts/mix_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402

NSAMP = 64_000_000
REPEATS = 9
T = gpsiq.MixTerm


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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mix_rates.txt")
    assert torch.cuda.is_available(), "the measurement needs the MI355X"
    ctx = gpsiq.Context(0)
    torch.manual_seed(64)
    x8 = torch.randint(-128, 128, (2 * NSAMP,), dtype=torch.int8, device="cuda")
    x16 = torch.randint(-32768, 32768, (2 * NSAMP,), dtype=torch.int16, device="cuda")
    y8 = torch.randint(-128, 128, (2 * NSAMP,), dtype=torch.int8, device="cuda")
    work = torch.empty(4 * NSAMP, dtype=torch.uint8, device="cuda")              # dst of every shape; the in-place stream is copied into it per call
    W = work.data_ptr()
    tone = T.tone(40, (37 << 50) + 11)
    swept = T.tone(-25, -(1 << 56), rate=(1 << 58) // 4099, sweep=(4099, 0))
    gated = T.tone(31, 5 << 52, gate=(2600, 650, 100))
    # (name, out format, the stream copied into dst before each call or None, terms, shift, qmax, bytes the terms read)
    shapes = [
        ("in place int8: stream + tone", SC08, x8, [T.stream(W, SC08, 1 << 6), tone], 6, 127, 2 * NSAMP),
        ("in place int16: stream + tone", SC16, x16, [T.stream(W, SC16, 1 << 6), T.tone(40 << 8, (37 << 50) + 11)], 6, 32767, 4 * NSAMP),
        ("repeater int16: stream + rotated (delay 701) + 2 tones", SC16, None,
         [T.stream(x16.data_ptr(), SC16, 1 << 7), T.rotated(x16.data_ptr(), SC16, 1, 3 << 49, skip=701), swept, gated], 8, 32767, 4 * NSAMP + 4 * (NSAMP - 701)),
        ("eight terms int8", SC08, None,
         [T.stream(x8.data_ptr(), SC08, 1 << 9), T.stream(x16.data_ptr(), SC16, 3), T.stream(y8.data_ptr(), SC08, -(1 << 8), skip=333),
          T.rotated(x8.data_ptr(), SC08, 2, 7 << 50, skip=64), T.rotated(y8.data_ptr(), SC08, -1, -(9 << 50), rate=1 << 40, sweep=(65, 0)), tone, swept, gated],
         10, 127, 2 * NSAMP + 4 * NSAMP + 2 * (NSAMP - 333) + 2 * (NSAMP - 64) + 2 * NSAMP),
    ]
    lines = [f"# python scripts/mix_rates.py: gpsiq_mix over one span of {NSAMP} samples, kernel id {gpsiq.kernels_id()}",
             f"# kernel_ms, median of {REPEATS} calls (the two kernels alternate call by call); copy: a device-to-device hipMemcpyAsync of the same byte count, measured in this run",
             "# shape | bytes moved MB | copy ms | generic ms | GB/s | / copy | rows ms | GB/s | / copy | rows / generic | default | default is the faster"]
    ok = True
    faster = {}
    for name, out_size, seed, terms, shift, qmax, read in shapes:
        moved = read + 2 * NSAMP * out_size
        ms = {"generic": [], "rows": []}
        res = {}
        for rep in range(REPEATS + 2):
            for k in ms:
                os.environ["GPSIQ_MIX_KERNEL"] = k
                if seed is not None:
                    work[:seed.numel() * seed.element_size()].copy_(seed.view(torch.uint8))
                clipped, t = ctx.mix(NSAMP, 12345, terms, shift, qmax, out_size, W)
                assert ctx.mix_last_plan()[0] == k
                if rep == 0:
                    res[k] = (clipped, work[:2 * NSAMP * out_size].clone())
                if rep >= 2:
                    ms[k].append(t)
        del os.environ["GPSIQ_MIX_KERNEL"]
        assert res["generic"][0] == res["rows"][0] and torch.equal(res["generic"][1], res["rows"][1]), name
        res.clear()
        if seed is not None:
            work[:seed.numel() * seed.element_size()].copy_(seed.view(torch.uint8))
        ctx.mix(NSAMP, 12345, terms, shift, qmax, out_size, W)
        default = ctx.mix_last_plan()[0]
        copy = copy_ms(moved // 2)
        med = {k: statistics.median(v) for k, v in ms.items()}
        fastest = min(med, key=med.get)
        faster[name] = fastest
        ok &= default == fastest
        cols = [f"{med[k]:.3f} | {moved / med[k] / 1e6:.0f} | {med[k] / copy:.2f}" for k in ("generic", "rows")]
        lines.append(f"{name} | {moved / 1e6:.0f} | {copy:.3f} | {cols[0]} | {cols[1]} | {med['rows'] / med['generic']:.3f} | {default} | {'yes' if default == fastest else 'NO'}")
        print(lines[-1], flush=True)
    lines.append("# the default path is the faster of the two at every row" if ok else "# the default path is NOT the faster at every row: see kMixRowsDefault")
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3] + lines[-1:]))


if __name__ == "__main__":
    main()
