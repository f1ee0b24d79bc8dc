"""profiles/pack_rates.txt: what packing costs.  The stream is the one of profiles/level_rates.txt -- 2.6 Msps int8, 16 channels, 4 130
blocks (2.15 GB), rendered by the levelled gpsiq_launch -- plus the int16 row (2 065 blocks, the same bytes).
  kernels    gpsiq_pack and gpsiq_unpack at 4 and 2 bits through their kernel_ms, the minimum of five.  The yardstick, in the same run: a
             device-to-device copy of the source bytes (torch's copy_ of a contiguous uint8 tensor: one asynchronous device-to-device
             memcpy) between events, the levelled gpsiq_launch of the same blocks, and the launch with level and noise off.
  batch      gpsiq_generate_batch_packed at 4 and 2 bits against gpsiq_generate_batch at GPSIQ_SC08 into the same page-locked host
             memory, level on, 4 130 blocks: wall time per call (the minimum of three) and bytes over the link.
usage: timeout -k 10 420 python scripts/pack_rates.py [out.txt]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import PK2, PK4, SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NCHAN = 2.6e6, 16
NSAMP = 260000


def copy_ms(dst, src):
    best = 1e9
    for _ in range(6):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dst.copy_(src)
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pack_rates.txt")
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    lines = [f"# packed streams: gpsiq_pack / gpsiq_unpack on a rendered device stream, kernel id {gpsiq.kernels_id()}; 2.6 Msps, 16 channels, 260 000 samples per block",
             "# kernels: stream | levelled launch ms | launch, level and noise off ms | device-to-device copy of the source ms | kernel | ms | / copy | source GB/s | bytes moved GB/s | clamped"]
    desc = synth_blocks(4130, NCHAN, seed=1)
    for name, ss, nb in (("int8 4130 blocks", SC08, 4130), ("int16 2065 blocks", SC16, 2065)):
        q = gpsiq.quantize_blocks(desc[:nb], FS, NSAMP)[0]
        ctx.set_descriptors(q)
        stride = 2 * NSAMP * ss
        src = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        other = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        ctx.noise_off()
        ctx.level_off()
        ctx.time_launches(0, nb, NSAMP, ss, src.data_ptr(), stride, 3, stream=s)
        off = min(ctx.time_launches(0, nb, NSAMP, ss, src.data_ptr(), stride, 10, stream=s) for _ in range(5))
        for bits in (PK4, PK2):
            qmax = 7 if bits == PK4 else 1
            ctx.set_noise(7, 1000.0, 0)
            ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], 1000.0), qmax / 3.0 if bits == PK4 else 1.0), qmax)
            ctx.time_launches(0, nb, NSAMP, ss, src.data_ptr(), stride, 3, stream=s)
            lev = min(ctx.time_launches(0, nb, NSAMP, ss, src.data_ptr(), stride, 10, stream=s) for _ in range(5))
            ctx.noise_off()
            ctx.level_off()
            cp = copy_ms(other, src)
            plen = gpsiq.packed_block_bytes(NSAMP, bits)
            packed = torch.empty(nb * plen, dtype=torch.uint8, device="cuda")
            ctx.pack(nb, NSAMP, ss, src.data_ptr(), stride, bits, packed.data_ptr(), plen, stream=s)
            runs = [ctx.pack(nb, NSAMP, ss, src.data_ptr(), stride, bits, packed.data_ptr(), plen, stream=s) for _ in range(5)]
            ms, clipped = min(r[1] for r in runs), runs[0][0]
            lines.append(f"{name} | {lev:.3f} | {off:.3f} | {cp:.3f} | pack {bits} bit | {ms:.3f} | {ms / cp:.3f} | {nb * stride / ms / 1e6:.0f} | {nb * (stride + plen) / ms / 1e6:.0f} | {clipped}")
            ctx.unpack(nb, NSAMP, bits, packed.data_ptr(), plen, ss, other.data_ptr(), stride, stream=s)
            ms = min(ctx.unpack(nb, NSAMP, bits, packed.data_ptr(), plen, ss, other.data_ptr(), stride, stream=s) for _ in range(5))
            lines.append(f"{name} | {lev:.3f} | {off:.3f} | {cp:.3f} | unpack {bits} bit | {ms:.3f} | {ms / cp:.3f} | {nb * stride / ms / 1e6:.0f} | {nb * (stride + plen) / ms / 1e6:.0f} | -")
            if ss == SC08 and clipped == 0:                     # the round trip of the levelled stream, while it is here
                assert torch.equal(other, src), "unpack(pack(x)) != x"
            del packed
        del src, other
    # the batch call
    lines.append("# batch: call, 4130 blocks into page-locked host memory, level on (noise sigma 1000) | wall ms per call | bytes over the link | GB/s of rendered stream")
    nb = 4130
    host = torch.empty(nb * 2 * NSAMP, dtype=torch.uint8).pin_memory()
    for label, bits in (("gpsiq_generate_batch GPSIQ_SC08", 0), ("gpsiq_generate_batch_packed 4 bit", PK4), ("gpsiq_generate_batch_packed 2 bit", PK2)):
        qmax = 1 if bits == PK2 else 7
        ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], 1000.0), qmax / 3.0 if qmax == 7 else 1.0), qmax)
        best = 1e9
        for _ in range(4):
            ctx.set_noise(7, 1000.0, 0)
            t0 = time.perf_counter()
            if bits:
                ctx.generate_batch_packed(desc, NSAMP, FS, bits, host_ptr=host.data_ptr())
            else:
                ctx.generate_batch(desc, NSAMP, FS, SC08, host_ptr=host.data_ptr())
            best = min(best, (time.perf_counter() - t0) * 1e3)
        link = nb * (gpsiq.packed_block_bytes(NSAMP, bits) if bits else 2 * NSAMP)
        pieces = ctx.pack_last_plan()[3] if bits else 0
        lines.append(f"{label}{f' ({pieces} pieces)' if bits else ''} | {best:.2f} | {link} | {nb * 2 * NSAMP / best / 1e6:.1f}")
    ctx.noise_off()
    ctx.level_off()
    ctx.close()
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
