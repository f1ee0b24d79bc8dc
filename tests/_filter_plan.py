"""The planner and the operand builder of the filter calls: tests/filter_plan.cpp (csrc/gpsiq_filter_plan.h, the header the calls themselves plan with)
compiled once per process with the host compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

Plan = collections.namedtuple("Plan", "kernel nout next grid threads run steps runs lds")
Nothing = collections.namedtuple("Nothing", "nout next")
Limits = collections.namedtuple("Limits", "min_taps max_tap max_run threads")
KERNELS = {0: "generic", 1: "mfma"}
AUTO, GENERIC, MFMA = 0, 1, 2                   # the `force` argument: what GPSIQ_FILTER_KERNEL names

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="filter_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "filter_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "filter_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nsamp, in_size, ntaps, decim, phase, max_tap, force) | ("piece", nblocks, nsamp, src_block_bytes,
    override) | ("planes", ntaps, decim, seed, kind) | ("limits",) -> Plan / Nothing / int / True / Limits per request; one process
    for all"""
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
            out.append(Nothing(int(kv["nout"]), int(kv["next"])))
        elif words[0] == "planes":
            out.append(words[1] == "ok")
        elif "kernel" in kv:
            out.append(Plan(*(int(kv[k]) for k in Plan._fields)))
        elif "piece" in kv:
            out.append(int(kv["piece"]))
        else:
            out.append(Limits(*(int(kv[k]) for k in Limits._fields)))
    return out


def plan(nsamp, in_size, ntaps, decim, phase, max_tap=0, force=AUTO):
    return ask([("plan", nsamp, in_size, ntaps, decim, phase, max_tap, force)])[0]


def limits():
    return ask([("limits",)])[0]
