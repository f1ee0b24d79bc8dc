"""Which kernel a launch takes: tests/plan_query.cpp (plan_synth() of csrc/gpsiq_launch_plan.h, the header the launcher itself
plans with) compiled once per process with the host compiler, and the SynthClass of a quantised descriptor array derived the way
gpsiq_set_descriptors does (csrc/gpsiq_device.cpp).  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")

ROWS_MAX_CODE_STEP = ((31 << 56) - 1) // 63          # kRowsMaxCodeStep
HALF_ROWS_MAX_CODE_STEP = ((31 << 56) - 1) // 31     # kHalfRowsMaxCodeStep

SynthClass = collections.namedtuple("SynthClass", "max_code_step max_active max_amplitude")
Plan = collections.namedtuple("Plan", "kernel stage variant rows wave_rows tiles big_wgs big_blocks tiles_small grid")

_exe = None


def executable():
    global _exe
    if _exe is None:
        d = tempfile.mkdtemp(prefix="plan_query_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "plan_query")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "plan_query.cpp")], check=True)
        _exe = exe
    return _exe


def synth_class(q):
    """q: QCHAN_DTYPE [nblocks][nchan].  Unused slots (prn 0) count for nothing; the amplitude bound is the largest per-block sum of
    (long)(250 * |gain|)."""
    q = np.asarray(q)
    used = q["prn"] != 0
    step = int(np.where(used, q["code_step"], 0).max()) if q.size else 0
    active = int(used.sum(axis=1).max()) if q.size else 0
    amp = np.where(used, np.trunc(250.0 * np.abs(q["gain"])), 0.0).astype(np.int64)
    return SynthClass(step, active, int(amp.sum(axis=1).max()) if q.size else 0)


def auto_variant(max_code_step):
    return "seg" if max_code_step <= ROWS_MAX_CODE_STEP else "segh" if max_code_step <= HALF_ROWS_MAX_CODE_STEP else "generic"


def _request(variant, ss, nsamp, nblocks, cls, max_z, level, env):
    """max_z: max |z| of the noise table, None while the noise is off.  env: where the process that launches reads the
    GPSIQ_SEG_* / GPSIQ_NO_FAST knobs (seg_policy_from_env)."""
    if variant == "auto":
        variant = auto_variant(cls.max_code_step)
    fast = 0 if int(env.get("GPSIQ_NO_FAST", "0") or 0) != 0 else 1
    knobs = [env.get(k, "-") for k in ("GPSIQ_SEG_TAIL_WGS", "GPSIQ_SEG_MAX_WAVE_ROWS", "GPSIQ_SEG_SETUP_ROWS", "GPSIQ_SEG_DRAIN")]
    return [str(x) for x in (variant, ss, nsamp, nblocks, cls.max_active, cls.max_amplitude, -1 if max_z is None else int(max_z),
                             1 if level else 0, fast)] + knobs


def _parse(line):
    if " ; " not in line:
        return Plan(line, None, None, 0, 0, 0, 0, 0, 0, 0)
    kernel, rest = line.split(" ; ")
    kv = dict(w.split("=") for w in rest.split())
    return Plan(kernel, kv["stage"], kv["variant"], *(int(kv[k]) for k in Plan._fields[3:]))


def query(variant, ss, nsamp, nblocks, cls, max_z=None, level=False, env=None):
    r = subprocess.run([executable()] + _request(variant, ss, nsamp, nblocks, cls, max_z, level, os.environ if env is None else env),
                       capture_output=True, text=True, check=True, timeout=60)
    return _parse(r.stdout.strip())


def query_many(requests):
    """requests: tuples of query()'s arguments (env last, a dict); one process for all of them."""
    text = "".join(" ".join(_request(*r)) + "\n" for r in requests)
    r = subprocess.run([executable(), "-"], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    return [_parse(s) for s in lines]
