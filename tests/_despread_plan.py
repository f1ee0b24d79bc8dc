"""Which correlator kernel a gpsiq_despread call takes: tests/despread_plan.cpp (plan_despread() of csrc/gpsiq_despread_plan.h, the
header the call itself plans with) compiled once per process with the host compiler; and the case table of the GPU tests
(tests/test_gpu_despread.py runs every case, tests/test_despread_ref.py holds the table against the planner on the CPU).
TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

import _plan_query as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")
SC08, SC16 = 1, 2

Plan = collections.namedtuple("Plan", "kernel slots grid threads tiles wave_rows seg_rows nseg")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="despread_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "despread_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "despread_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def _parse(line):
    if line.strip() == "nothing":
        return None
    kv = dict(w.split("=") for w in line.split())
    return Plan(kv["kernel"], *(int(kv[k]) for k in Plan._fields[1:]))


def query_many(requests, sanitize=False):
    """requests: (nsamp, nblocks, seg_len, max_code_step, max_active, force_generic, target_wgs or None); one process for all"""
    text = "".join("%d %d %d %d %d %d %s\n" % (r[0], r[1], r[2], r[3], r[4], 1 if r[5] else 0, "-" if r[6] is None else int(r[6])) for r in requests)
    r = subprocess.run([executable(sanitize), "-"], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    return [_parse(s) for s in lines]


def query(nsamp, nblocks, seg_len, cls, force=False, target=None, sanitize=False):
    return query_many([(nsamp, nblocks, seg_len, cls.max_code_step, cls.max_active, force, target)], sanitize)[0]


def kernel_name(plan, ss):
    """the instantiation behind a plan, as csrc/gpsiq_despread_kernels.hip spells it"""
    return "despread_generic<%d>" % ss if plan.kernel == "generic" else "despread_rows<%d, %d>" % (ss, plan.slots)


INSTANTIATIONS = sorted(["despread_generic<%d>" % ss for ss in (SC08, SC16)] +
                        ["despread_rows<%d, %d>" % (ss, n) for ss in (SC08, SC16) for n in (4, 8, 12, 16)])

# ---- the GPU case table -------------------------------------------------------------------------------------------------------
# active: which of the nchan input slots hold a satellite ("x") -- gaps make device order differ from input order; a list gives
# every resident block its own pattern.  nres blocks are resident, the call works on [block0, block0 + nblocks).  guard: bytes
# between the blocks of the stream, filled with 0x7f.  force: GPSIQ_DESPREAD_KERNEL=generic; target: GPSIQ_DESPREAD_TARGET_WGS.
Case = collections.namedtuple("Case", "name fs ss nchan active nsamp nres block0 nblocks seg_len guard force target kernel")

LONG = 70001                       # crosses a data-bit edge at 2.6 Msps (20 ms = 52 000 samples)
LONG_ROWS = (LONG + 63) // 64      # 1094


def _table():
    t = []

    def add(name, fs, ss, active, nsamp, seg_len, nres=2, block0=0, nblocks=None, guard=0, force=False, target=None, kernel="rows"):
        pats = active if isinstance(active, list) else [active] * nres
        assert len(pats) == nres and len({len(p) for p in pats}) == 1
        t.append(Case(name, fs, ss, len(pats[0]), pats, nsamp, nres, block0, nres - block0 if nblocks is None else nblocks, seg_len,
                      guard, force, target, kernel))

    # lengths: one sample, either side of a row, either side of a chunk of 64 rows, a data-bit edge; both formats in turn
    for i, n in enumerate([1, 63, 64, 65, 4095, 4097, LONG]):
        add("len-%d" % n, 2.6e6, (SC08, SC16)[i & 1], "xx.xx.x", n, 2560, guard=64 if i & 2 else 0)
    # segments at the default grid of one 70 001-sample block: 5 workgroups, every wave one chunk of 64 rows
    for seg in (64, 128, 2560, 70016, 1 << 30):
        add("seg-%d" % seg, 2.6e6, SC16 if seg != 128 else SC08, "xxxx", LONG, seg, nres=1)
    # ... and with waves of 256 rows (four chunks): a segment edge inside a wave's run (and inside a chunk), on a wave edge, on a
    # workgroup edge.  wave_rows comes from the planner (asserted on the CPU): 256 at a target of one workgroup
    for name, rows in (("inside-run", 88), ("wave-edge", 256), ("wg-edge", 1024)):
        add("seg-" + name, 2.6e6, SC16 if name != "wave-edge" else SC08, "xxxxx", LONG, 64 * rows, nres=2, target=1, guard=4)
    # channels: every slot count of the row kernel, filled and not, unused slots in between, a block with no channel at all
    add("ch-1", 2.6e6, SC16, "...x", 4097, 2560)
    add("ch-4", 2.6e6, SC08, "xxxx", 4097, 2560)
    add("ch-5", 2.6e6, SC08, ".x.xx.xx", 4097, 128)
    add("ch-8", 2.6e6, SC16, "xxxxxxxx", 4097, 128)
    add("ch-12", 2.6e6, SC16, "xxxxxxxxxxxx", 4097, 2560)
    add("ch-12-int8", 2.6e6, SC08, "x.xxxxxx.xxxxx", 4097, 2560)
    add("ch-16", 2.6e6, SC16, "x" * 16, 8191, 2560, guard=128)
    add("ch-16-int8", 2.6e6, SC08, "x" * 16, 8191, 64)
    add("ch-none", 2.6e6, SC16, ["xx.x", "....", "x..x"], 4097, 2560, nres=3)
    add("blocks-7", 2.6e6, SC08, "x.xx.x", 4160, 2560, nres=9, block0=2, nblocks=7, guard=32)
    # rates: generic below 2.08 Msps, rows above; one shape through both kernels
    add("rate-0.8", 0.8e6, SC16, "xxx.xx", 8001, 2560, kernel="generic")
    add("rate-0.8-int8", 0.8e6, SC08, "x" * 16, 4161, 128, kernel="generic", guard=4)
    add("rate-1.5", 1.5e6, SC08, "xxxxxxxxx", 8001, 64, kernel="generic")
    add("rate-25", 25e6, SC16, "xxxxxxxxx", 20001, 2560)
    add("both-rows", 2.6e6, SC16, "xxxx.xx", 20001, 2560, guard=8)
    add("both-generic", 2.6e6, SC16, "xxxx.xx", 20001, 2560, guard=8, force=True, kernel="generic")
    add("both-rows-int8", 2.6e6, SC08, "xxxx.xx", 20001, 2560)
    add("both-generic-int8", 2.6e6, SC08, "xxxx.xx", 20001, 2560, force=True, kernel="generic")
    return t


CASES = _table()


def case_class(c):
    """the SynthClass of a case's resident set as gpsiq_set_descriptors derives it, without quantising: the code step is
    f_code / fs * 2^56 with f_code within 1.023e6 +- 5 Hz (gpsiq.scenario.synth_blocks), far from either kernel's limit"""
    step = int(round(1.023e6 / c.fs * 2.0 ** 56))
    return pq.SynthClass(step, max(p.count("x") for p in c.active), 0)


def case_env(c):
    env = {}
    if c.force:
        env["GPSIQ_DESPREAD_KERNEL"] = "generic"
    if c.target is not None:
        env["GPSIQ_DESPREAD_TARGET_WGS"] = str(c.target)
    return env
