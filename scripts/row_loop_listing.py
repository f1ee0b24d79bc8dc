"""profiles/<tag>_synth_tile_row_loop.txt: the row loop of the SHIPPED default kernels, disassembled.

Pulls the gfx950 code objects out of multi-sdr-gps-sim_amd/gpsiq/libgpsiq.so (clang offload bundles in .hip_fatbin), runs
llvm-objdump -d on them, finds synth_tile<1, 16, 64, 1, true, 8, false> (int8) and synth_tile<2, ...> (int16), and prints
the innermost loop that holds the per-channel core (the ds_read_b32 gathers): every instruction with the issue cost of its
encoding class as measured on this chip (profiles/r01_ubench_valu_encodings.txt), and the totals the roofline discussion in
DESIGN.md section 4 quotes (VALU per 16-channel row, LDS gathers, issue cycles).  No GPU needed.
A second argument is a regular expression that selects other kernels by their demangled name, e.g. the headline kernels of the
noise and the output level: 'synth_tile_(noise|level)<[12], 16, 64, 1, true>'.
usage: python scripts/row_loop_listing.py [tag [kernel-regex]]

--hashes: one line per kernel whose demangled name matches the regex (default: every synth_tile / synth_tile_noise instantiation),
with the SHA-256 prefix of its instruction stream (llvm-objdump -d, addresses and comments stripped).  With a second library the
two are compared kernel by kernel: how a change is shown to have left existing kernels as they were (build the commit before
with `make -C multi-sdr-gps-sim_amd/csrc OUT=<elsewhere>/libgpsiq.so` and pass that file).
usage: python scripts/row_loop_listing.py --hashes [--regex R] [library [library-before]]"""
import hashlib
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "gpsiq", "libgpsiq.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CXXFILT = "c++filt"

# issue cycles per wave instruction, measured (profiles/r01_ubench_valu_encodings.txt): plain VOP2 with VGPR operands 2.5;
# SGPR-operand / VOP3 / SDWA / packed forms 4.3; v_lshl_add_u64 4.4
def issue_cycles(op, text):
    if not op.startswith("v_"):
        return None
    if op == "v_lshl_add_u64":
        return 4.4
    if "sdwa" in op or op.endswith("_e64") or op.startswith("v_pk_") or op in ("v_add3_u32", "v_lshl_add_u32", "v_perm_b32", "v_and_or_b32", "v_bfe_u32", "v_alignbit_b32", "v_mad_u32_u24"):
        return 4.3
    if re.search(r"\bs\d+|\bs\[\d+:\d+\]|\bvcc|\bexec", text.split(None, 1)[1] if " " in text else ""):
        return 4.3
    return 2.5


def code_objects(lib=None):
    blob = open(lib or LIB, "rb").read()
    out = []
    for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob):
        base = m.start()
        (n,) = struct.unpack_from("<Q", blob, base + 24)
        p = base + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                out.append(blob[base + off: base + off + size])
    return out


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "r05"
    pattern = sys.argv[2] if len(sys.argv) > 2 else r"synth_tile<[12], 16, 64, 1, true, 8, false>"
    dst = os.path.join(ROOT, "profiles", f"{tag}_synth_tile_row_loop.txt")
    lines_out = []
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects()):
            path = os.path.join(td, f"co{k}.o")
            open(path, "wb").write(co)
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout
            funcs = re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", dis)
            for f in funcs:
                head = f.split("\n", 1)[0]
                m = re.match(r"[0-9a-f]+ <([^>]+)>:", head)
                if not m:
                    continue
                name = subprocess.run([CXXFILT, m.group(1)], capture_output=True, text=True).stdout.strip()
                if not re.search(pattern, name):
                    continue
                body = [ln.strip() for ln in f.split("\n")[1:] if ln.strip()]
                ins = []
                for ln in body:
                    t = ln.split("//")[0].strip()
                    addr = re.search(r"//\s*([0-9A-Fa-f]+):", ln)
                    if t:
                        ins.append((int(addr.group(1), 16) if addr else None, t))
                # the innermost loops whose body holds the LDS gathers; of those the one with the most of them: the whole-trip loop
                # (several rows per pass) where there is one, rather than the single-row loop of the remainder rows
                best = None
                backward = []
                for i, (a, t) in enumerate(ins):
                    mm = re.match(r"s_cbranch_\w+\s+(\d+)", t) or re.match(r"s_branch\s+(\d+)", t)
                    if not mm or a is None:
                        continue
                    tgt = a + 4 + 4 * (int(mm.group(1)) - (1 << 16 if int(mm.group(1)) >= 1 << 15 else 0))
                    j = next((q for q, (aa, _) in enumerate(ins) if aa == tgt), None)
                    if j is None or j > i:
                        continue
                    backward.append((j, i))
                for j, i in backward:
                    if any((j2, i2) != (j, i) and j <= j2 and i2 <= i for j2, i2 in backward):
                        continue                                # another loop inside: not innermost
                    seg = ins[j:i + 1]
                    gathers = sum(1 for _, x in seg if x.startswith("ds_read_b32"))
                    if gathers >= 16 and (best is None or gathers > sum(1 for _, x in best if x.startswith("ds_read_b32"))):
                        best = seg
                lines_out.append(f"== {name}")
                if best is None:
                    lines_out.append("   (row loop not found: the loop heuristics want updating)")
                    continue
                cls = collections.Counter()
                cyc = 0.0
                for a, t in best:
                    op = t.split()[0]
                    c = issue_cycles(op, t)
                    kind = "VALU" if op.startswith("v_") else "LDS" if op.startswith("ds_") else "VMEM" if op.startswith(("global_", "buffer_", "flat_")) else "SALU/other"
                    cls[kind] += 1
                    if c:
                        cyc += c
                    lines_out.append(f"   {a:08x}  {t:<64s} {'' if c is None else f'{c:.1f}'}")
                gathers = sum(1 for _, x in best if x.startswith("ds_read_b32"))
                wide = sum(1 for _, x in best if x.startswith("ds_read_b128"))
                rows = max(cls['VMEM'], 1)                      # one store per row
                lines_out.append(f"   -- one pass of the loop = {rows} 64-sample row(s) of 16 channels: {cls['VALU']} VALU ({cls['VALU'] / rows:.2f} per row, "
                                 f"{cls['VALU'] / rows / 16:.2f} per channel-row), {gathers} ds_read_b32 gathers + {wide} ds_read_b128, {cls['VMEM']} store(s), "
                                 f"{cls['SALU/other']} scalar / wait / branch / scheduling mark; "
                                 f"VALU issue at the measured rates: {cyc / rows:.1f} cycles per row = {cyc / rows / 16:.2f} per channel-row")
    hdr = [f"# row loop of the default kernels in the shipped libgpsiq.so (kernel id {kernels_id()}), llvm-objdump -d; right column: issue cycles of the",
           "# instruction's encoding class as measured on MI355X (profiles/r01_ubench_valu_encodings.txt: VOP2 on VGPRs 2.5, SGPR-operand / VOP3 /",
           "# SDWA / packed 4.3, v_lshl_add_u64 4.4).  Regenerate: python scripts/row_loop_listing.py <tag>", ""]
    open(dst, "w").write("\n".join(hdr + lines_out) + "\n")
    print(dst, len(lines_out), "lines")
    for ln in lines_out:
        if ln.startswith("==") or ln.startswith("   --"):
            print(ln)


def kernel_hashes(lib, pattern):
    """{demangled kernel name (without the parameter list): hash of its instructions}"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for k, co in enumerate(code_objects(lib)):
            path = os.path.join(td, f"co{k}.o")
            open(path, "wb").write(co)
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True).stdout
            funcs = {}
            for f in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", dis):
                m = re.match(r"[0-9a-f]+ <([^>]+)>:", f.split("\n", 1)[0])
                if m:
                    # ("...": the zero padding up to the next function's alignment, which depends on the order of the functions in the
                    # code object, not on this one's instructions)
                    funcs[m.group(1)] = [t for t in (ln.split("//")[0].strip() for ln in f.split("\n")[1:]) if t and t != "..."]
            names = list(funcs)
            dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
            for n, d in zip(names, dem):
                if re.search(pattern, d):
                    # (a kernel in an anonymous namespace keeps its name: the first "(" of it is not its parameter list's)
                    out[d.replace("(anonymous namespace)", "{anonymous}").split("(")[0]] =(hashlib.sha256("\n".join(funcs[n]).encode()).hexdigest()[:16], len(funcs[n]))
    return out


def hashes_main(argv):
    pattern = r"synth_tile(_noise)?<"
    if argv[:1] == ["--regex"]:
        pattern, argv = argv[1], argv[2:]
    now = kernel_hashes(argv[0] if argv else LIB, pattern)
    before = kernel_hashes(argv[1], pattern) if len(argv) > 1 else None
    same = 0
    for name in sorted(set(now) | set(before or {})):
        h, n = now.get(name, ("-", 0))
        if before is None:
            print(f"{h} {n:5d}  {name}")
            continue
        hb, nb = before.get(name, ("-", 0))
        same += h == hb
        print(f"{h} {n:5d}  {hb} {nb:5d}  {'same' if h == hb else 'DIFFERENT'}  {name}")
    if before is not None:
        print(f"# {same} of {len(set(now) | set(before))} kernels matching {pattern!r} have the same instructions in both libraries")
        return 0 if same == len(set(now) | set(before)) else 1
    return 0


def kernels_id():
    sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd"))
    import gpsiq
    return gpsiq.kernels_id()


if __name__ == "__main__":
    if sys.argv[1:2] == ["--hashes"]:
        sys.exit(hashes_main(sys.argv[2:]))
    main()
