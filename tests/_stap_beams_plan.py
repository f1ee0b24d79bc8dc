"""The planner of gpsiq_stap_beams, the digit planes of its matrix kernel and a CPU model of one of that kernel's chunks:
tests/stap_beams_plan.cpp (csrc/gpsiq_stap_beams_plan.h, the header the call itself plans with) compiled once per process with the host
compiler, plain and with -fsanitize=address,undefined.  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

GENERIC, MFMA = 0, 1
KERNELS = {GENERIC: "generic", MFMA: "mfma"}
AUTO, FORCE_GENERIC, FORCE_MFMA = 0, 1, 2
FORCE = {"generic": FORCE_GENERIC, "mfma": FORCE_MFMA, None: AUTO}

Plan = collections.namedtuple("Plan", "kernel padded grid threads run runs can")
Split = collections.namedtuple("Split", "planes generic")
Tile = collections.namedtuple("Tile", "peak acc")
Limits = collections.namedtuple("Limits", "max_beams max_entry chunk8 chunk16 tile8 tile16 max_grid gen_grid threads never coef_dwords")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="stap_beams_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "stap_beams_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "stap_beams_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def ask(requests, sanitize=False):
    """requests: tuples ("plan", nelem, ntaps, nbeams, nsamp, in_size, out_size, max_entry, force) | ("split", lo, hi) | ("minrows", in_size, nbeams) |
    ("planes", nelem, ntaps, nbeams, seed, kind) | ("tile", nelem, ntaps, nbeams, in_size, out_size, nsamp, seed, kind, heads) |
    ("limits",) -> Plan / None (nothing is launched) / Split / the rows / True / Tile / Limits per request; one process for all"""
    text = "".join(" ".join(str(int(v)) if i else v for i, v in enumerate(r)) + "\n" for r in requests)
    r = subprocess.run([executable(sanitize)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    out = []
    for s in lines:
        words = s.split()
        kv = dict(w.split("=") for w in words if "=" in w)
        if words[0] == "nothing":
            out.append(None)
        elif "rows" in kv and len(kv) == 1:
            out.append(int(kv["rows"]))
        elif words[0] == "planes":
            assert words[1] == "ok"
            out.append(True)
        elif words[0] in ("split", "tile"):
            assert words[1] == "ok"
            kind = Split if words[0] == "split" else Tile
            out.append(kind(*(int(kv[k]) for k in kind._fields)))
        else:
            kind = Plan if "kernel" in kv else Limits
            out.append(kind(*(int(kv[k]) for k in kind._fields)))
    return out


def limits():
    return ask([("limits",)])[0]


def padded_taps(nelem, ntaps):
    """csrc/gpsiq_stap_beams_geometry.h, beams_padded_taps, restated: the next power of two while nelem times it fits 32 rows, else 0"""
    tp = 1 if ntaps <= 1 else 2 if ntaps <= 2 else 4 if ntaps <= 4 else 8
    return tp if nelem * tp <= 32 else 0


def default_is_mfma(in_size, padded_rows, nbeams):
    """csrc/gpsiq_stap_beams_plan.h, beams_mfma_min_rows, restated from profiles/stap_beams_rates.txt: eight beams from 2 (int8 input)
    or 8 (int16) padded rows on, four to seven beams from 8 or 16, fewer beams never"""
    if nbeams >= 8:
        return padded_rows >= (2 if in_size == 1 else 8)
    return nbeams >= 4 and padded_rows >= (8 if in_size == 1 else 16)
