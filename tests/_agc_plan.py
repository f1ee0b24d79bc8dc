"""The planner of the gain control calls: tests/agc_plan.cpp (csrc/gpsiq_agc_plan.h, the header the calls themselves plan with, and the
gain rule of csrc/gpsiq_agc_geometry.h) compiled once per process with the host compiler, plain and with -fsanitize=address,undefined.
TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

Plan = collections.namedtuple("Plan", "nwin next measure gains apply threads units cnt zero mult mask scratch")
Span = collections.namedtuple("Span", "nwin next")
Limits = collections.namedtuple("Limits", "threads unit tile apply_tile tile_windows lead_units")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="agc_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "agc_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "agc_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nsamp, window, fill, mask) | ("span", nsamp, window, fill) | ("gain", sumsq, count, target_q8, mult0,
    mult_min, mult_max) | ("piece", nblocks, nsamp, src_block_bytes, override) | ("limits",) -> Plan or None / Span / int / int / Limits
    per request; one process for all"""
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
        elif "measure" in kv:
            out.append(Plan(*(int(kv[k]) for k in Plan._fields)))
        elif "nwin" in kv:
            out.append(Span(int(kv["nwin"]), int(kv["next"])))
        elif "gain" in kv:
            out.append(int(kv["gain"]))
        elif "piece" in kv:
            out.append(int(kv["piece"]))
        else:
            out.append(Limits(*(int(kv[k]) for k in Limits._fields)))
    return out


def plan(nsamp, window, fill=0, mask=False):
    return ask([("plan", nsamp, window, fill, mask)])[0]


def limits():
    return ask([("limits",)])[0]
