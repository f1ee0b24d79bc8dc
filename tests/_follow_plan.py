"""How a gpsiq_follow call is cut into launches: tests/follow_plan.cpp (plan_follow() of csrc/gpsiq_follow_plan.h, the header the call
itself plans with) compiled once per process with the host compiler; and the case table of the GPU tests (tests/test_gpu_follow.py
runs every case, tests/test_follow_ref.py holds the table's claims against the restatement on the CPU).  TEST INFRASTRUCTURE."""
import atexit
import collections
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-sdr-gps-sim_amd", "csrc")
SC08, SC16 = 1, 2
PER_LAUNCH = 4096

Plan = collections.namedtuple("Plan", "grid threads per_launch records record_bytes max_launches launches")

_exe = {}


def executable(sanitize=False):
    if sanitize not in _exe:
        d = tempfile.mkdtemp(prefix="follow_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "follow_plan")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                        os.path.join(ROOT, "tests", "follow_plan.cpp")], check=True)
        _exe[sanitize] = exe
    return _exe[sanitize]


def query_many(requests, sanitize=False):
    """requests: (nsamp, sample_size, nprn, max_epochs, knob or None, most records of any satellite); one process for all"""
    text = "".join("%d %d %d %d %d %d\n" % (r[0], r[1], r[2], r[3], r[4] or 0, r[5]) for r in requests)
    r = subprocess.run([executable(sanitize), "-"], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests), r.stderr
    return [None if s.strip() == "nothing" else Plan(*(int(w.split("=")[1]) for w in s.split())) for s in lines]


def query(nsamp, ss, nprn, max_epochs, knob=None, records=0, sanitize=False):
    return query_many([(nsamp, ss, nprn, max_epochs, knob, records)], sanitize)[0]


# ---- the GPU case table -------------------------------------------------------------------------------------------------------------
# One call per case.  base: the stream's first byte modulo 16; guard: bytes of 0x7f behind the span; stream: "random" (random elements,
# the format's extremes at both ends), "min", "max" or "zero"; cfg and every state: keyword arguments of _follow_ref.make_cfg /
# make_state; cut: (satellite, k) -- the span is shortened to end exactly on the last sample of that satellite's record k; expect: the
# statuses the restatement must give (None: not pinned), so that a case is what its name says.
Case = collections.namedtuple("Case", "name ss base guard nsamp stream cfg states max_epochs cut expect")

C15 = 3 << 55                     # 1.5 chips a sample: an epoch of 682 samples
LOOP = dict(kf=1 << 44, kp=1 << 40, ki=1 << 36, kd=1 << 42, pull_epochs=10)       # the loops switch mid-run
STILL = dict(kf=0, kp=0, ki=0, kd=0, pull_epochs=0)                                 # nothing moves the steps
TOP56 = (1 << 56) - 1


def _table():
    t = []

    def add(name, ss, states, nsamp=27500, cfg=LOOP, max_epochs=64, base=0, guard=64, stream="random", cut=None, expect=None):
        t.append(Case(name, ss, base, guard, nsamp, stream, dict(cfg), [dict(s) for s in states], max_epochs, cut, expect))

    three = [dict(prn=5, code_step=C15, carr_step=123456789012345),
             dict(prn=12, sample=1, chip=300, code_frac=12345, code_step=C15, carr_step=-(1 << 50)),
             dict(prn=5, sample=777, chip=1022, code_frac=TOP56 - 4, code_step=C15)]                     # a satellite twice, an epoch of one sample
    five = three + [dict(prn=32, sample=12, chip=511, code_frac=1 << 55, code_step=C15, carr_step=-987654321),
                    dict(prn=1, sample=13, chip=1, code_step=C15 + 99991, code_step0=C15, carr_step=1 << 40, carr_int=(1 << 40) + 5, prev=(-4000000, 1 << 22), epoch=9)]
    add("mixed-int16", SC16, three, expect=(1, 1, 1))
    add("mixed-int8", SC08, five, base=4, guard=16, expect=(1,) * 5)
    add("base12-int8", SC08, three[:2], base=12, guard=4)
    add("base12-int16", SC16, three[1:], base=12, guard=256)
    # first epochs of 128, 129, 127 samples, of 65 (two rows) and of 64 (one)
    add("lengths", SC16, [dict(prn=7, chip=c, code_step=1 << 56, sample=s) for c, s in ((895, 0), (894, 1), (896, 2), (958, 3), (959, 5))], nsamp=6000, max_epochs=5,
        base=4, expect=(2,) * 5)
    add("lengths-int8", SC08, [dict(prn=7, chip=c, code_step=1 << 56, sample=s) for c, s in ((895, 1), (894, 0), (896, 3), (958, 2), (959, 7))], nsamp=3200, max_epochs=5,
        base=4)
    # the ends of the code step's range: 512 samples an epoch, and 16368
    add("step-max", SC08, [dict(prn=3, code_step=(1 << 57) - 1, carr_step=4321), dict(prn=4, sample=9, chip=1000, code_step=(1 << 57) - 1)], nsamp=3000, cfg=STILL,
        expect=(1, 1))
    add("step-min", SC16, [dict(prn=3, code_step=1 << 52, carr_step=5000), dict(prn=9, sample=3, chip=512, code_step=1 << 52, carr_step=-5000)], nsamp=2 * 16368 + 100,
        cfg=STILL, max_epochs=4, expect=(1, 1))
    # taps: the late tap reaches back across the period; a spacing of a whole chip and of one unit
    add("late-wrap", SC16, [dict(prn=21, code_frac=1000, code_step=C15), dict(prn=21, sample=5, code_frac=(1 << 55) - 1, code_step=C15)], nsamp=9000, guard=0)
    add("spacing-chip", SC08, [dict(prn=30, code_step=C15), dict(prn=30, chip=1022, code_frac=TOP56, code_step=C15)], nsamp=9000, cfg=dict(LOOP, spacing=1 << 56))
    add("spacing-one", SC16, [dict(prn=30, code_step=C15), dict(prn=2, chip=5, code_step=C15)], nsamp=9000, cfg=dict(LOOP, spacing=1))
    # carrier: steps whose N * w wraps 2^59 hundreds of times, one of them negative
    add("carrier", SC16, [dict(prn=14, code_step=C15, carr_step=-(1 << 57) - 999), dict(prn=29, sample=1, code_step=C15, carr_step=(1 << 57) + 12345)],
        cfg=dict(LOOP, kf=1 << 30), nsamp=14000, expect=(1, 1))
    # pull-in only, phase lock only
    add("pull-never", SC08, three[:2], cfg=dict(LOOP, pull_epochs=0), nsamp=14000)
    add("pull-always", SC16, three[:2], cfg=dict(LOOP, pull_epochs=1000), nsamp=14000)
    # stops: a first epoch that does not fit, a start at and past the end of the span, the span ending on an epoch's last sample, a full array
    add("no-room", SC16, [dict(prn=8, sample=6900, code_step=C15), dict(prn=8, code_step=C15), dict(prn=8, sample=7000, code_step=C15),
                          dict(prn=8, sample=7005, code_step=C15)], nsamp=7000, expect=(1, 1, 1, 1))
    add("exact-end", SC08, three[:2], cut=(0, 11), base=8, guard=8, expect=(1, 1))
    add("full", SC16, three, max_epochs=7, expect=(2, 2, 2))
    # a step driven out of its range while the others run on; a step out of range on entry
    add("range-code", SC16, [dict(prn=17, code_step=(1 << 57) - 1000), dict(prn=17, code_step=C15), dict(prn=18, code_step=(1 << 52) + 1000, chip=1000)],
        cfg=dict(LOOP, kd=(1 << 46) - 1), nsamp=9000, expect=(3, 1, 3))
    add("range-carrier", SC08, [dict(prn=17, code_step=C15, carr_step=(1 << 58) - (1 << 41)), dict(prn=17, code_step=C15, carr_step=-(1 << 58) + (1 << 41)),
                                dict(prn=19, code_step=C15)], cfg=dict(LOOP, kf=(1 << 46) - 1, pull_epochs=1000), nsamp=27500, expect=None)
    add("range-entry", SC08, [dict(prn=6, code_step=1 << 57, code_step0=C15), dict(prn=6, code_step=C15, carr_step=1 << 58, carr_int=0), dict(prn=6, code_step=C15),
                              dict(prn=6, code_step=(1 << 52) - 1, code_step0=C15)], nsamp=3000, expect=(3, 3, 1, 3))
    # streams of one value: the format's minimum (whose negation overflows it), its maximum, and zero (every zero denominator)
    for kind in ("min", "max", "zero"):
        for ss in (SC08, SC16):
            add("%s-int%d" % (kind, 8 * ss), ss, three[:2], nsamp=7000, stream=kind, base=4 * ss, expect=(1, 1))
    return t


CASES = _table()
