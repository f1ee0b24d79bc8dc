"""Which kernels a gpsiq_acquire call takes: tests/acquire_plan.cpp (plan_acquire() of csrc/gpsiq_acquire_plan.h, the header the call
itself plans with) compiled once per process with the host compiler; and the case table of the GPU tests (tests/test_gpu_acquire.py
runs every case, tests/test_acquire_ref.py holds the table against the planner on the CPU).  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")
SC08, SC16 = 1, 2

Plan = collections.namedtuple("Plan", "kernel digits span cells corr_cells gx gy gz row_tiles npad scratch wipe_grid mx my mz ksteps lds peak_grid")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="acquire_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "acquire_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "acquire_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def _parse(line):
    if line.strip() == "nothing":
        return None
    kv = dict(w.split("=") for w in line.split())
    return Plan(kv["kernel"], *(int(kv[k]) for k in Plan._fields[1:]))


def query_many(requests, sanitize=False):
    """requests: (nsamp, sample_size, nprn, ndopp, nshift, ncoh, nnoncoh, hop, force) with force None, "generic", "mfma" or "nofast";
    one process for all"""
    text = "".join("%d %d %d %d %d %d %d %d %s\n" % (tuple(r[:8]) + (r[8] or "-",)) for r in requests)
    r = subprocess.run([executable(sanitize), "-"], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    return [_parse(s) for s in lines]


def query(nsamp, ss, nprn, ndopp, nshift, ncoh, nnoncoh, hop, force=None, sanitize=False):
    return query_many([(nsamp, ss, nprn, ndopp, nshift, ncoh, nnoncoh, hop, force)], sanitize)[0]


def span_of(nshift, ncoh, nnoncoh, hop):
    return (nshift - 1) + (nnoncoh - 1) * hop + ncoh


# ---- the GPU case table -------------------------------------------------------------------------------------------------------------
# Every case is run with GPSIQ_ACQUIRE_KERNEL=mfma (the matrix path wherever it can serve, also below a full tile, whatever the library's
# default) and again with GPSIQ_ACQUIRE_KERNEL=generic.  base: the stream's first byte modulo 16; guard:
# bytes of 0x7f behind the span.  prns: the list searched.  step: (carr_step0, carr_step_inc) or None for 500 Hz bins centred on 0.
Case = collections.namedtuple("Case", "name ss prns ndopp nshift ncoh nnoncoh hop base guard step")

ALL32 = tuple(range(1, 33))


def full_tile(ndopp, nshift):
    """where the planner takes the matrix path by default (if it is the default at all)"""
    return ndopp >= 2 and nshift >= 256


def _table():
    t = []

    def add(name, ss, prns, ndopp, nshift, ncoh, nnoncoh=1, hop=None, base=0, guard=0, step=None):
        hop = ncoh if hop is None else hop
        t.append(Case(name, ss, tuple(prns), ndopp, nshift, ncoh, nnoncoh, hop, base, guard, step))

    # shifts either side of a tile's 16 columns and of a wave's 256 shifts, against every coherent length, bin count and format in turn
    i = 0
    for nshift in (1, 15, 16, 17, 255, 256, 257):
        for ncoh in (64, 128, 320):
            ndopp = (1, 2, 3, 6)[i % 4]
            # (base and guard step on their own cycles of 5 and 7 cases: every bin count and coherent length meets several of each)
            add("s%d-c%d-d%d" % (nshift, ncoh, ndopp), (SC08, SC16)[(i // 2) & 1], [(5, 12, 30)[i % 3]], ndopp, nshift, ncoh, base=4 * ((i // 5 + i) % 4),
                guard=(0, 4, 64, 12, 256, 8, 1024)[i % 7])
            i += 1
    # every bin count with both digit counts on the matrix path: row tiles full and partly filled
    for ndopp in (2, 3, 6):
        for ss in (SC08, SC16):
            add("rows-d%d-ss%d" % (ndopp, ss), ss, [9, 1, 32], ndopp, 257, 128, base=(8, 0, 12, 4)[(ndopp + ss) % 4], guard=512)
    # dwells, with the hop below, equal to and above the coherent length, a hop that is no multiple of 16 and one that is odd
    for nn, hop in ((2, 64), (2, 128), (3, 200), (3, 129), (3, 127), (2, 16)):
        add("k%d-h%d" % (nn, hop), (SC08, SC16)[hop & 1], [17, 22, 4], 3, 257 if hop != 16 else 300, 128, nn, hop, base=12 if hop & 1 else 4, guard=2048)
        add("k%d-h%d-generic-shape" % (nn, hop), SC16, [17], 1, 17, 128, nn, hop)
    # satellite lists of one, three and all 32
    add("prn-32", SC08, ALL32, 2, 256, 64, 2, 100, guard=4)
    add("prn-32-int16", SC16, ALL32, 3, 272, 64)
    add("prn-twice", SC16, [11, 11, 2], 2, 256, 64)
    # a negative first bin with bins that straddle zero, and a step between bins so large that m * step wraps 2^59 many times
    add("negative", SC16, [8, 23], 6, 300, 320, 2, 333, base=4, step=(-(5 << 47) - 12345, (2 << 47) + 777))
    add("negative-int8", SC08, [8], 5, 260, 128, step=(-(1 << 58) + 1, (1 << 56) + 3))
    add("wraps", SC16, [14, 29], 4, 256, 192, 2, 192, step=((1 << 58) - 1, -(1 << 57) - 99991))
    add("wraps-generic-shape", SC08, [14], 3, 40, 192, 2, 192, step=((1 << 58) - 1, -(1 << 57) - 99991))
    return t


CASES = _table()


def case_steps(c):
    """(code_step, carr_step0, carr_step_inc)"""
    code = int(round(1.023e6 / 2.6e6 * 2.0 ** 56))
    if c.step is None:
        inc = int(round(500.0 / 2.6e6 * 2.0 ** 59))
        return code, -(c.ndopp // 2) * inc, inc
    return (code,) + tuple(c.step)
