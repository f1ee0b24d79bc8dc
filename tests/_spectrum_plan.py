"""The planner of gpsiq_spectrum: tests/spectrum_plan.cpp (csrc/gpsiq_spectrum_plan.h, the header the call itself plans with) compiled
once per process with the host compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

Plan = collections.namedtuple("Plan", "kernel nseg ngroups grid threads run per work lds power_bytes")
Nothing = collections.namedtuple("Nothing", "nseg ngroups")
Limits = collections.namedtuple("Limits", "default_mfma run max_grid mfma_grid max_shift")
KERNELS = {0: "generic", 1: "mfma"}
AUTO, GENERIC, MFMA = 0, 1, 2                   # the `force` argument: what GPSIQ_SPECTRUM_KERNEL names

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="spectrum_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "spectrum_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "spectrum_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nsamp, sample_size, nfft, hop, navg, force) | ("fits", sample_size, nfft, window, navg, shift) |
    ("minshift", sample_size, nfft, window, navg) | ("limits",) -> Plan / Nothing / bool / int / Limits per request; one process"""
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
            out.append(Nothing(int(kv["nseg"]), int(kv["ngroups"])))
        elif "kernel" in kv:
            out.append(Plan(*(int(kv[k]) for k in Plan._fields)))
        elif "fits" in kv:
            out.append(kv["fits"] == "1")
        elif "shift" in kv:
            out.append(int(kv["shift"]))
        else:
            out.append(Limits(*(int(kv[k]) for k in Limits._fields)))
    return out


def plan(nsamp, sample_size, nfft, hop, navg, force=AUTO):
    return ask([("plan", nsamp, sample_size, nfft, hop, navg, force)])[0]


def limits():
    return ask([("limits",)])[0]
