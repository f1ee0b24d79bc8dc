"""profiles/r07_noise_rates.txt: what receiver noise costs the synthesis kernel.  gpsiq_launch on resident descriptors, timed with
noise off and on (sigma 1000), for the headline config (2.6 Msps int8, 16 channels, 4 130 blocks) and int16 at 2.6, 10 and 25 Msps
(about 2 GB of output per launch); then the row loop of the noise kernel (scripts/row_loop_listing.py's view of it).
usage: python scripts/noise_rates.py [out.txt]      (needs the MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))

import torch  # noqa: E402

import gpsiq  # noqa: E402
from gpsiq.abi import SC08, SC16  # noqa: E402
from gpsiq.scenario import synth_blocks  # noqa: E402

CONFIGS = [("2.6 Msps int8 16 ch 4130 blocks (headline)", 2.6e6, SC08, 4130),
           ("2.6 Msps int16 16 ch 2065 blocks", 2.6e6, SC16, 2065),
           ("10 Msps int16 16 ch 500 blocks", 10e6, SC16, 500),
           ("25 Msps int16 16 ch 200 blocks", 25e6, SC16, 200)]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07_noise_rates.txt")
    ctx = gpsiq.Context(0)
    lines = [f"# receiver noise: gpsiq_launch (default variant) on resident descriptors, noise off vs on (sigma 1000), kernel id {gpsiq.kernels_id()}",
             "# config | off ms | on ms | off G samples/s | on G samples/s | on / off (rate)"]
    for name, fs, ss, nb in CONFIGS:
        nsamp = int(round(fs / 10))
        desc = synth_blocks(nb, 16, seed=1)
        q = gpsiq.quantize_blocks(desc, fs, nsamp)[0]
        ctx.set_descriptors(q)
        stride = 2 * nsamp * ss
        buf = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        res = []
        for sigma in (0.0, 1000.0):
            ctx.set_noise(7, sigma, 0)
            ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 3, stream=s)               # warm-up
            ms = min(ctx.time_launches(0, nb, nsamp, ss, buf.data_ptr(), stride, 10, stream=s) for _ in range(5))
            res.append(ms)
        gs = [nb * nsamp / (m * 1e-3) / 1e9 for m in res]
        lines.append(f"{name} | {res[0]:.3f} | {res[1]:.3f} | {gs[0]:.1f} | {gs[1]:.1f} | {res[0] / res[1]:.3f}")
        del buf
    ctx.close()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import re
    import subprocess
    import tempfile
    import row_loop_listing as L
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(L.code_objects()):
            p = os.path.join(td, f"co{k}.o")
            open(p, "wb").write(co)
            dis = subprocess.run([L.OBJDUMP, "-d", "--no-show-raw-insn", p], capture_output=True, text=True).stdout
            for f in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", dis):
                m = re.match(r"[0-9a-f]+ <([^>]+)>:", f.split("\n", 1)[0])
                if not m:
                    continue
                name = subprocess.run([L.CXXFILT, m.group(1)], capture_output=True, text=True).stdout.strip()
                if not re.search(r"synth_tile_noise<1, 16, 64, 1, true>", name):
                    continue
                body = [re.sub(r"\s*//.*", "", ln).strip() for ln in f.split("\n")[1:]]
                ins = [b for b in body if b]
                # the row loop: from the first of the 16 gathers' loop head to its backward branch (the longest run holding
                # 16 ds_read_b32 and ending in s_cbranch)
                best = None
                for i, t in enumerate(ins):
                    if t.startswith("s_cbranch") and sum(1 for x in ins[max(0, i - 400):i] if x.startswith("ds_read_b32")) >= 16:
                        j = i
                        while j > 0 and not ins[j - 1].startswith(("s_cbranch", "s_branch")):
                            j -= 1
                        seg = ins[j:i + 1]
                        if sum(1 for x in seg if x.startswith("ds_read_b32")) >= 16 and (best is None or len(seg) < len(best)):
                            best = seg
                lines.append(f"\n== {name}: row loop ({'not found' if best is None else len(best)} instructions)")
                if best:
                    valu = sum(1 for x in best if x.startswith("v_"))
                    lds = sum(1 for x in best if x.startswith("ds_"))
                    lines.append(f"   {valu} VALU, {lds} LDS per 64-sample row of 16 channels")
                    lines += ["   " + x for x in best]
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:8]))


if __name__ == "__main__":
    main()
