"""The dispatches behind a fixed list of gpsiq_launch calls, for comparing two commits' launchers on the device.

  render:   rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python scripts/launch_dispatches.py render
            every variant x int8 / int16 x 4 / 8 / 12 / 16 active channels at 2.6 Msps (26 blocks), then the default variant at
            1.023 Msps (segh), 0.8 Msps (generic), 25 Msps, with the noise on, with the level on, on a 1-block and on a 2000-block set
  compare:  python scripts/launch_dispatches.py compare BEFORE_DIR AFTER_DIR [summary.txt]
            the gpsiq kernels of the two traces in dispatch order: kernel name, grid size, workgroup size and LDS size must be equal
(kernel trace only: no counters in that run.  Needs the MI355X for `render`; the script sets no time limit of its own.)"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))


def launches():
    out = []
    for variant in range(9):
        for ss in (1, 2):
            for nchan in (4, 8, 12, 16):
                out.append((2.6e6, ss, nchan, 26, variant, 0.0, False))
    for fs, nb in ((1.023e6, 26), (0.8e6, 26), (25e6, 26), (2.6e6, 1), (2.6e6, 2000)):
        out.append((fs, 1, 16, nb, 0, 0.0, False))
        out.append((fs, 2, 16, nb, 0, 0.0, False))
    for ss in (1, 2):
        out.append((2.6e6, ss, 16, 26, 0, 1000.0, False))
        out.append((2.6e6, ss, 16, 26, 0, 0.0, True))
        out.append((2.6e6, ss, 16, 26, 0, 1000.0, True))
    return out


def render():
    import torch
    import gpsiq
    from gpsiq.scenario import synth_blocks
    ctx = gpsiq.Context(0)
    s = torch.cuda.current_stream().cuda_stream
    for fs, ss, nchan, nb, variant, sigma, level in launches():
        nsamp = int(round(fs / 10))
        desc = synth_blocks(nb, nchan, seed=1)
        ctx.set_descriptors(gpsiq.quantize_blocks(desc, fs, nsamp)[0])
        stride = 2 * nsamp * ss
        buf = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
        ctx.set_noise(7, sigma, 0)
        qmax = 127 if ss == 1 else 32767
        if level:
            ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], sigma), qmax / 3.0), qmax)
        else:
            ctx.level_off()
        ctx.launch(0, nb, nsamp, ss, buf.data_ptr(), stride, stream=s, variant=variant)
        ctx.synchronize(s)
        del buf
    ctx.close()
    print(len(launches()), "launches rendered")


def dispatches(d):
    paths = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, (d, paths)
    rows = list(csv.DictReader(open(paths[0])))
    rows = [r for r in rows if "gpsiq::" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    keys = [k for k in rows[0] if k == "Kernel_Name" or k.startswith("Grid_Size") or k.startswith("Workgroup_Size") or k.startswith("LDS")]
    return keys, [tuple(r[k] for k in keys) for r in rows]


def compare(before, after, out=None):
    ka, a = dispatches(before)
    kb, b = dispatches(after)
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    lines = [f"# gpsiq kernel dispatches of scripts/launch_dispatches.py render ({len(launches())} launches), rocprofv3 --kernel-trace: before | after",
             f"# compared per dispatch, in dispatch order: {' '.join(ka)}",
             f"dispatches: {len(a)} | {len(b)}", f"distinct kernels: {len({x[0] for x in a})} | {len({x[0] for x in b})}",
             f"differing dispatches: {len(diff) + abs(len(a) - len(b))}"]
    for i, x, y in diff[:20]:
        lines.append(f"  #{i}: {x} | {y}")
    lines.append("EQUAL" if ka == kb and a == b else "NOT EQUAL")
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text, end="")
    return 0 if ka == kb and a == b else 1


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    elif len(sys.argv) == 2 and sys.argv[1] == "render":
        render()
    else:
        sys.exit(__doc__)
