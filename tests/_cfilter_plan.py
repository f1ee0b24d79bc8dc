"""The planner and the operand builder of gpsiq_cfilter: tests/cfilter_plan.cpp (csrc/gpsiq_cfilter_plan.h, the header the call itself
plans with) compiled once per process with the host compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

GENERIC, MFMA, MFMA16 = 0, 1, 2
KERNELS = {GENERIC: "generic", MFMA: "mfma", MFMA16: "mfma16"}
AUTO, FORCE_GENERIC, FORCE_MFMA = 0, 1, 2
FORCE = {"generic": FORCE_GENERIC, "mfma": FORCE_MFMA, None: AUTO}

Plan = collections.namedtuple("Plan", "kernel nout next grid threads run steps runs lds")
Nothing = collections.namedtuple("Nothing", "nout next")
Limits = collections.namedtuple("Limits", "min_taps8 min_taps16 max_tap max_run min_run16 lds threads")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="cfilter_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "cfilter_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "cfilter_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nsamp, in_size, ntaps, decim, phase, max_re, max_im, min_im, force) | ("planes", in_size, ntaps, decim,
    seed, kind) | ("limits",) -> Plan or Nothing / True / Limits per request; one process for all"""
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
        else:
            out.append(Limits(*(int(kv[k]) for k in Limits._fields)))
    return out


def stats(taps):
    """(max_re, max_im, min_im) of taps [n, 2]: what the planner looks at"""
    return int(taps[:, 0].max()), int(taps[:, 1].max()), int(taps[:, 1].min())


def plan(nsamp, in_size, ntaps, decim, phase, taps_stats=(0, 0, 0), force=AUTO):
    return ask([("plan", nsamp, in_size, ntaps, decim, phase) + tuple(taps_stats) + (force,)])[0]


def limits():
    return ask([("limits",)])[0]
