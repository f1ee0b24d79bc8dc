"""The planner of the mix calls: tests/mix_plan.cpp (csrc/gpsiq_mix_plan.h, the header the calls themselves plan with) compiled once
per process with the host compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

Plan = collections.namedtuple("Plan", "kernel grid threads lead units")
Limits = collections.namedtuple("Limits", "rows_default threads max_grid slot_bytes max_terms max_shift")
KERNELS = {0: "generic", 1: "rows"}
AUTO, GENERIC, ROWS = 0, 1, 2                   # the `force` argument: what GPSIQ_MIX_KERNEL names

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="mix_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "mix_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "mix_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nsamp, m0, out_size, dst_addr, force) | ("piece", nblocks, nsamp, block_bytes, override) |
    ("limits",) -> Plan / None (nothing is launched) / int / Limits per request; one process for all"""
    text = "".join(" ".join(str(int(v)) if i else v for i, v in enumerate(r)) + "\n" for r in requests)
    r = subprocess.run([executable(sanitize)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    out = []
    for s in lines:
        words = s.split()
        kv = dict(w.split("=") for w in words if "=" in w)
        if words[0] == "nothing":
            out.append(None)
        elif "kernel" in kv:
            out.append(Plan(*(int(kv[k]) for k in Plan._fields)))
        elif "piece" in kv:
            out.append(int(kv["piece"]))
        else:
            out.append(Limits(*(int(kv[k]) for k in Limits._fields)))
    return out


def plan(nsamp, m0, out_size, dst_addr=0, force=AUTO):
    return ask([("plan", nsamp, m0, out_size, dst_addr, force)])[0]


def limits():
    return ask([("limits",)])[0]
