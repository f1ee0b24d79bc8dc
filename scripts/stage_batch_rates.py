"""Wall time per call of the four staged batch calls, the batch leg of scripts/pack_rates.py for all of them
(profiles/stage_batch_rates.txt is a table of this script's lines: the parent commit's library, this one's, the parent's again).  2.6 Msps int8, 16 channels, 4 130 blocks of 260 000 samples (2.15 GB of rendered stream) into page-locked host memory,
level on (noise sigma 1000):
  gpsiq_generate_batch GPSIQ_SC08         the plain call, for continuity with profiles/pack_rates.txt
  gpsiq_generate_batch_packed             4 and 2 bits
  gpsiq_generate_batch_filtered           65 taps, decimated by 2, int8 out
  gpsiq_generate_batch_mixed              the stream plus one tone, in place
  gpsiq_generate_batch_resampled          2.6 to 2.048 Msps, 128 phases of 16 taps, interpolated, int8 out
time.perf_counter() round the call, the best of four after one untimed call (so that the context's staging exists), and the piece
count of the call's last plan.  GPSIQ_LIB names the library, as for every program that imports gpsiq.  ONLY: a word of a call's
name (packed, filtered, mixed, resampled) -- the context then makes no other staged call, so the call's streams are the first ones
made for such calls in the process, whichever library is loaded.
usage: timeout -k 10 300 python scripts/stage_batch_rates.py [out.txt [ONLY]]      (needs the MI355X; the script sets no time limit of its own)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import PK2, PK4, SC08  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

FS, NCHAN, NSAMP, NB = 2.6e6, 16, 260000, 4130


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None                  # the lines go to stdout either way
    only = sys.argv[2] if len(sys.argv) > 2 else ""
    ctx = gpsiq.Context(0)
    desc = synth_blocks(NB, NCHAN, seed=1)
    host = torch.empty(NB * 2 * NSAMP, dtype=torch.uint8).pin_memory()
    ptr = host.data_ptr()
    ftaps = gpsiq.filter_design(FS, 0.9e6, 65, 14)
    step = gpsiq.resample_step(FS, 2.048e6)
    rtaps = gpsiq.resample_design(step, 0.8, 7, 16, 14)
    tone = gpsiq.MixTerm.tone(9, 37 << 50)                              # amplitude 9 * 250 / 2^6 = 35
    calls = (
        ("gpsiq_generate_batch GPSIQ_SC08", 7, lambda: ctx.generate_batch(desc, NSAMP, FS, SC08, host_ptr=ptr), None),
        ("gpsiq_generate_batch_packed 4 bit", 7, lambda: ctx.generate_batch_packed(desc, NSAMP, FS, PK4, host_ptr=ptr), ctx.pack_last_plan),
        ("gpsiq_generate_batch_packed 2 bit", 1, lambda: ctx.generate_batch_packed(desc, NSAMP, FS, PK2, host_ptr=ptr), ctx.pack_last_plan),
        ("gpsiq_generate_batch_filtered 65 taps decim 2", 127, lambda: ctx.generate_batch_filtered(desc, NSAMP, FS, SC08, ftaps, 14, 2, SC08, host_ptr=ptr),
         ctx.filter_last_plan),
        ("gpsiq_generate_batch_mixed 1 tone", 127, lambda: ctx.generate_batch_mixed(desc, NSAMP, FS, SC08, 1 << 6, [tone], 6, 127, host_ptr=ptr), ctx.mix_last_plan),
        ("gpsiq_generate_batch_resampled to 2.048 Msps", 127,
         lambda: ctx.generate_batch_resampled(desc, NSAMP, FS, SC08, rtaps, 7, 14, 1, step, 0, SC08, host_ptr=ptr, capacity=NB * NSAMP), ctx.resample_last_plan),
    )
    lines = [f"# staged batch calls, kernel id {gpsiq.kernels_id()}; 2.6 Msps int8, 16 channels, {NB} blocks of {NSAMP} samples into page-locked host memory, "
             "level on (noise sigma 1000)" + (f"; a context that makes the {only} call only" if only else ""),
             "# call | pieces | wall ms per call (best of 4 after one warm call) | GB/s of rendered stream"]
    for label, qmax, call, plan in calls:
        if only not in label:
            continue
        ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], 1000.0), qmax / 3.0 if qmax > 1 else 1.0), qmax)
        best = 1e9
        for k in range(5):
            ctx.set_noise(7, 1000.0, 0)
            t0 = time.perf_counter()
            call()
            if k:
                best = min(best, (time.perf_counter() - t0) * 1e3)
        lines.append(f"{label} | {plan()[3] if plan else '-'} | {best:.2f} | {NB * 2 * NSAMP / best / 1e6:.1f}")
    ctx.noise_off()
    ctx.level_off()
    ctx.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
