"""The planner of the pack / unpack calls: tests/pack_plan.cpp (csrc/gpsiq_pack_plan.h, the header the calls themselves plan with)
compiled once per process with the host compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

Plan = collections.namedtuple("Plan", "grid threads units tiles total unit_src unit_dst")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="pack_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "pack_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "pack_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("pack", nblocks, nsamp, sample_size, bits) | ("unpack", nblocks, nsamp, bits, sample_size) |
    ("piece", nblocks, src_block_bytes, override) | ("bytes", nsamp, bits) -> Plan / None / int per request; one process for all"""
    text = "".join(" ".join(str(int(v)) if i else v for i, v in enumerate(r)) + "\n" for r in requests)
    r = subprocess.run([executable(sanitize)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    out = []
    for s in lines:
        if s == "nothing":
            out.append(None)
            continue
        kv = dict(w.split("=") for w in s.split())
        out.append(Plan(*(int(kv[k]) for k in Plan._fields)) if "grid" in kv else int(next(iter(kv.values()))))
    return out
