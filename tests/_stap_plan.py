"""The planner of gpsiq_stap_cov / gpsiq_stap_combine and the host's way from the Gram tiles to the covariance: tests/stap_plan.cpp
(csrc/gpsiq_stap_plan.h, the header the calls themselves plan with) compiled once per process with the host compiler, plain and with
-fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

GENERIC, MFMA, COMBINE = 0, 1, 2
KERNELS = {GENERIC: "generic", MFMA: "mfma", COMBINE: "combine"}
AUTO, FORCE_GENERIC, FORCE_MFMA = 0, 1, 2

CovPlan = collections.namedtuple("CovPlan", "kernel groups grid threads run runs steps")
CombinePlan = collections.namedtuple("CombinePlan", "grid threads lead slots")
Gram = collections.namedtuple("Gram", "peak flushes tiles")
Limits = collections.namedtuple("Limits", "max_elem max_taps max_rows k flush min_run max_grid gen_run gen_grid chunk min_rows threads comb_grid gram_words")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="stap_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "stap_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "stap_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("cov", nelem, ntaps, nsamp, in_size, force) | ("combine", nsamp, out_size, dst_low4) |
    ("gram", nelem, ntaps, nsamp, seed, kind, heads) | ("limits",) -> CovPlan / CombinePlan / None (nothing is launched) / Gram / Limits
    per request; one process for all"""
    text = "".join(" ".join(str(int(v)) if i else v for i, v in enumerate(r)) + "\n" for r in requests)
    r = subprocess.run([executable(sanitize)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    out = []
    for s in lines:
        words = s.split()
        kv = dict(w.split("=") for w in words if "=" in w)
        if words[0] == "nothing":
            out.append(None)
        elif words[0] == "gram":
            assert words[1] == "ok"
            out.append(Gram(int(kv["peak"]), int(kv["flushes"]), int(kv["tiles"])))
        else:
            kind = CovPlan if "kernel" in kv else CombinePlan if "lead" in kv else Limits
            out.append(kind(*(int(kv[k]) for k in kind._fields)))
    return out


def limits():
    return ask([("limits",)])[0]
