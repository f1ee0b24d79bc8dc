"""Every noise and level kernel against the oracle at ragged and edge shapes: what tests/test_gpu_parity.py does for the plain
synth_tile family, for synth_tile_noise, synth_tile_level and synth_generic with a stage on.  Bit-exact; no tolerances.

The reference is composed from parts the suite already trusts, never from the library's own output (tests/_stage_cases.py,
compose()): S = the oracle's noiseless wrapped int16 sums, z = tests/_noise_ref.py, then the wrapping int16 / int8 store or
tests/_level_ref.py.  Every render is an explicit launch on resident descriptors into a 0x5A-filled buffer whose stride is larger
than a block; the stride padding and the bytes behind the last block must stay 0x5A; every set is launched whole and once more from
resident block 1, with the noise numbered next_block + block0.  Before a launch is compared the plan query (tests/_plan_query.py)
must name the kernel the case was written for.

The cases that need another process environment (GPSIQ_NO_FAST=1 for the int8 packed noise core, the GPSIQ_SEG_* grid-shape knobs for
waves of several chunks with a tail of one-chunk workgroups; the library reads them once per process) run in one child process per
environment: this file run as a script.  Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "multi-sdr-gps-sim_amd"), os.path.join(ROOT, "tests")]

import _noise_ref as nr
import _oracle
import _plan_query as pq
import _stage_cases as sc
import gpsiq
from _stage_cases import LEVEL, LEVEL_NOISE, NOISE, STAGES, Settings
from gpsiq.abi import NCO_FIXED, QCHAN_DTYPE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

VARIANTS = ["tile", "seg", "segh", "generic"]
QMAX = {SC08: (1, 7, 127), SC16: (2047, 32767)}
MULTS = (1, 40000, 65536, 200001, 2 ** 24 - 1)
GAINS = (0.0, -0.7, 1.0, 0.3333, 2.0, -300.0, 1e-3, 17.25)
# a small sigma, a large one and, where the level stage can represent it, one whose max |z| exceeds 32767
SIGMAS = {NOISE: (37.5, 1600.0), LEVEL_NOISE: (37.5, 1600.0, 15718.0), LEVEL: (None,)}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


class Resident:
    """A descriptor set, its class, its noiseless sums S (once) and the noise of its blocks (once per setting)."""

    def __init__(self, orc, q, nsamp):
        if q.shape[0] == 1:                                 # a single block is resident twice, so that a launch can start at block 1
            q = np.concatenate([q, q])
        self.q, self.nsamp, self.cls = q, nsamp, pq.synth_class(q)
        self.S = np.stack([orc.block_fixed(q[b], nsamp, SC16) for b in range(q.shape[0])])
        self._z = {}

    def want(self, ss, st, block0, nb):
        z = None
        if st.sigma is not None:
            key = (st.seed, st.sigma, st.next_block)
            if key not in self._z:
                self._z[key] = nr.noise(st.seed, st.sigma, st.next_block, self.q.shape[0], self.nsamp)
            z = self._z[key][block0:block0 + nb]
        return sc.compose(self.S[block0:block0 + nb], z, ss, st.level)


def apply(ctx, st):
    ctx.set_nco_mode(NCO_FIXED)
    if st.sigma is None:
        ctx.noise_off()
    else:
        ctx.set_noise(st.seed, st.sigma, st.next_block)
    if st.level is None:
        ctx.level_off()
    else:
        ctx.set_level(*st.level)


def run_device(ctx, nsamp, ss, variant, block0, nb):
    """tests/test_gpu_parity.py's run_device with a stride that is always larger than the block"""
    import torch
    blk = 2 * nsamp * ss
    stride = ((blk + 15) & ~15) + 16
    buf = torch.full((nb * stride + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.launch(block0, nb, nsamp, ss, buf.data_ptr(), stride, stream=torch.cuda.current_stream().cuda_stream, variant=gpsiq.variants()[variant])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[nb * stride:] == 0x5A).all(), "kernel wrote past the ring"
    rows = host[: nb * stride].reshape(nb, stride)
    assert (rows[:, blk:] == 0x5A).all(), "kernel wrote into the stride padding"
    return np.ascontiguousarray(rows[:, :blk]).view(np.int8 if ss == SC08 else np.int16)


def check(ctx, res, ss, variant, st, kernel, what):
    """Plan, then render resident blocks [0, nb) and [1, nb) and compare every element.  kernel: the name the launch must take.
    The plan is plan_synth() on the class tests/_plan_query.py derives from the descriptors, as gpsiq_set_descriptors derives its own:
    the assertion holds the case (and, where `kernel` comes from fast_core(), this file's restatement of the plain-add rule) to the
    planner header.  It does not observe the launch: that the library plans with the same class is what synth_class() mirrors."""
    nb_all = res.q.shape[0]
    apply(ctx, st)
    ctx.set_descriptors(res.q)
    stage = "noise" if st.level is None else "level"
    for block0 in (0, 1):
        nb = nb_all - block0
        plan = pq.query(variant, ss, res.nsamp, nb, res.cls, None if st.sigma is None else sc.max_z(st.sigma), st.level is not None)
        assert (plan.kernel, plan.stage) == (kernel, stage), (what, block0, plan)
        got = run_device(ctx, res.nsamp, ss, variant, block0, nb)
        want = res.want(ss, st, block0, nb)
        for b in range(nb):
            bad = np.nonzero(got[b] != want[b])[0]
            assert bad.size == 0, (f"{what}: {plan.kernel} block {block0}+{b}: {bad.size} of {want[b].size} elements differ, first at {bad[:8]}: "
                                   f"got {got[b][bad[:8]]} want {want[b][bad[:8]]}")
    return plan


def fast_core(cls, ss, st):
    """the plain-add rule of DESIGN.md 8a / 8b: with the level on the bound is on the signal alone and both formats run the int16
    cores; with the noise alone int8 keeps its 12-bit fields and int16 needs the bound on |I + zI|"""
    if st.level is not None:
        return cls.max_amplitude <= 32767
    return ss == SC08 or cls.max_amplitude + sc.max_z(st.sigma) <= 32767


def kernel_for(res, stage, ss, variant, st):
    return sc.kernel_of(stage, ss, res.cls.max_active, variant, fast_core(res.cls, ss, st))


def stage_settings(stage, ss, mi, qi, si, seed=0x57A6E, next_block=5000):
    """noise / level of a test: multiplier mi, clamp qi and sigma si of the lists (each index wraps on its own list).  One seed and
    block number per test, so that a descriptor set draws its noise once per sigma."""
    sigma = SIGMAS[stage][si % len(SIGMAS[stage])]
    level = None if stage == NOISE else (MULTS[mi % len(MULTS)], QMAX[ss][qi % len(QMAX[ss])])
    return Settings(seed, sigma, next_block, level)


class Sweep:
    """what the settings of a test reached, per stage and format"""

    def __init__(self):
        self.seen = set()

    def add(self, stage, ss, st, fast):
        self.seen.add((stage, ss, st.sigma, st.level, fast))

    def reached(self, stage, ss, fast=None):
        hit = [(sigma, level) for s_, f_, sigma, level, fa in self.seen if (s_, f_) == (stage, ss) and fast in (None, fa)]
        return {sg for sg, _ in hit}, {lv[0] for _, lv in hit if lv}, {lv[1] for _, lv in hit if lv}

    def assert_whole(self, cores):
        """every sigma of the stage, every multiplier and every clamp of the format, per stage and format; on each of `cores`"""
        for stage in STAGES:
            for ss in (SC08, SC16):
                for fast in cores:
                    if (stage, ss, fast) == (NOISE, SC08, False):
                        # int8 noise alone takes the plain-add core whatever the gains (the packed one: GPSIQ_NO_FAST=1, in the
                        # child process of test_cases_that_need_their_own_process)
                        assert not self.reached(stage, ss, fast)[0]
                        continue
                    sigmas, mults, qmaxs = self.reached(stage, ss, fast)
                    assert sigmas == set(SIGMAS[stage]), (stage, ss, fast, sigmas)
                    if stage != NOISE:
                        assert mults == set(MULTS) and qmaxs == set(QMAX[ss]), (stage, ss, fast, mults, qmaxs)


# ---- the case table: every instantiation ------------------------------------------------------------------------------------------

def run_case(ctx, orc, c):
    assert {k: os.environ.get(k) for k in sc.ENVS[c.env]} == sc.ENVS[c.env], "the case needs its process environment"
    res = Resident(orc, sc.descriptors(c), c.nsamp)
    plan = check(ctx, res, c.ss, c.variant, sc.settings(c), sc.kernel_name(c), c.name)
    if c.env == "grid":                                     # (the plan of the launch from block 1: two blocks, the second one the tail)
        assert plan.wave_rows > plan.rows and plan.wave_rows % plan.rows and 0 < plan.big_blocks < c.nblocks - 1, plan


@pytest.mark.parametrize("case", [c for c in sc.CASES if not c.env], ids=lambda c: c.name)
def test_every_instantiation_at_a_ragged_length(ctx, orc, case):
    run_case(ctx, orc, case)


def test_cases_that_need_their_own_process():
    """GPSIQ_NO_FAST=1: the eight int8 packed noise kernels; the grid-shape knobs: waves of several chunks, the last one partial, the
    block ending inside it, and a tail of one-chunk workgroups, for both families, both layouts, both cores, 4 / 8 / 12 slots.  One
    child after the other; the first that does not end well is the last one started."""
    for env in [e for e in sc.ENVS if e]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), env], env=dict(os.environ, **sc.ENVS[env]), capture_output=True, text=True,
                           timeout=600)
        n = len([c for c in sc.CASES if c.env == env])
        assert r.returncode == 0 and f"all {n} ok" in r.stdout, (env, r.returncode, (r.stdout + r.stderr)[-4000:])


# ---- ragged block lengths ---------------------------------------------------------------------------------------------------------

RAGGED_LENGTHS = [1, 63, 64, 65, 2047, 2049, 16383, 16384, 16385, 40000, 70001]


@pytest.mark.parametrize("nsamp", RAGGED_LENGTHS)
def test_ragged_block_lengths(ctx, orc, nsamp):
    d = synth_blocks(2, 7, seed=nsamp + 1)
    q, _ = gpsiq.quantize_blocks(d, 2.6e6, nsamp)
    res = Resident(orc, q, nsamp)
    i = RAGGED_LENGTHS.index(nsamp)
    for k, stage in enumerate(STAGES):
        for ss in (SC08, SC16):
            st = stage_settings(stage, ss, i + k, i, i, next_block=5000 + i)
            for variant in VARIANTS:
                check(ctx, res, ss, variant, st, sc.kernel_of(stage, ss, 7, variant, True), (stage, ss, variant, nsamp))


# ---- raw quantised descriptors ----------------------------------------------------------------------------------------------------

def fuzz_set(rng, half, nc, gains):
    """tests/test_gpu_parity.py's generators (test_quantised_descriptor_fuzz; test_half_row_kernel_fuzz when half): the same field
    ranges; prn 0 also in random places, so that the blocks of a set have different active counts"""
    max_step = pq.HALF_ROWS_MAX_CODE_STEP if half else pq.ROWS_MAX_CODE_STEP
    nb, nc = int(rng.integers(1, 4)), nc or int(rng.integers(1, 17))
    ns = int(rng.choice([1, 31, 33, 2047, 2049, 4999, 16384, 16385, 70001]))
    q = np.zeros((nb, nc), dtype=QCHAN_DTYPE)
    q["prn"] = rng.integers(0, 33, size=(nb, nc))
    q["prn"][rng.random((nb, nc)) < 0.2] = 0
    q["carr_phase"] = rng.integers(0, 1 << 59, size=(nb, nc), dtype=np.uint64)
    q["carr_step"] = rng.integers(-(1 << 58) + 1, 1 << 58, size=(nb, nc))
    q["code_frac"] = rng.integers(0, 1 << 56, size=(nb, nc), dtype=np.uint64)
    q["code_step"] = rng.integers(max_step // 2 if half else 1, max_step + 1, size=(nb, nc), dtype=np.uint64)
    q["code_step"][0, :] = max_step                                 # the limit itself
    q["chip0"] = rng.integers(0, 1023, size=(nb, nc))
    q["chip0"][:, ::3] = 1022
    q["icode"] = rng.integers(0, 20, size=(nb, nc))
    q["nav_bits"] = rng.integers(0, 1 << 32, size=(nb, nc), dtype=np.uint64).astype(np.uint32)
    q["gain"] = rng.choice(gains, size=(nb, nc))
    return q, ns


# per set: the channel slots (None: 1 .. 16 at random) and the gains.  A set that may draw -300 or 17.25 is past the amplitude bound
# in nearly every draw (the packed cores); every other set draws from the gains that keep 16 channels far inside it.
FUZZ_SETS = [(None, GAINS), (4, GAINS[:5] + GAINS[6:7]), (7, GAINS), (12, GAINS[:5] + GAINS[6:7]), (16, GAINS), (None, GAINS[:5] + GAINS[6:7])]


@pytest.mark.parametrize("variant", VARIANTS)
def test_quantised_descriptor_fuzz(ctx, orc, variant):
    """Random QUANTISED descriptors under every stage: full-range carrier steps, code steps to the kernel's limit, chips next to the
    period end, negative / zero / huge gains, unused slots anywhere, 1-3 blocks with different active counts.  The sets alternate
    between gains past the amplitude bound and gains inside it (the packed and the plain-add cores).  Every set goes through every
    multiplier while the clamp and the sigma step with the periods of their own lists, shifted from one pair of sets to the next:
    per stage, format and core every sigma of SIGMAS, every multiplier of MULTS and every clamp of QMAX is reached, which is
    asserted at the end."""
    rng = np.random.default_rng(3100 + VARIANTS.index(variant))
    slots, sweep = set(), Sweep()
    for case, (nc, gains) in enumerate(FUZZ_SETS):
        q, ns = fuzz_set(rng, variant in ("segh", "generic"), nc, gains)
        res = Resident(orc, q, ns)
        slots.add(sc.slots_of(res.cls.max_active))
        pair = case // 2                                    # sets 2p and 2p + 1: the same settings on either core
        for stage in STAGES:
            for ss in (SC08, SC16):
                for j in range(len(MULTS) if stage != NOISE else len(SIGMAS[NOISE])):
                    st = stage_settings(stage, ss, j, j + pair, j + pair, next_block=5000 + case)
                    fast = fast_core(res.cls, ss, st)
                    check(ctx, res, ss, variant, st, kernel_for(res, stage, ss, variant, st), (variant, case, stage, ss, ns, q.shape, st))
                    sweep.add(stage, ss, st, fast)
    assert sc.max_z(SIGMAS[LEVEL_NOISE][2]) > 32767
    sweep.assert_whole((False, True))
    assert len(slots) >= 3


# ---- boundary phases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_boundary_phases(ctx, orc, variant):
    """tests/test_gpu_parity.py's test_boundary_phases set (phases exactly on chip / LUT / period / nav-bit / word boundaries, zero and
    extreme Doppler, binary-fraction rates at 4.092 Msps) under each stage, with every sigma, multiplier and clamp; the set is resident
    twice, so that a launch starts at block 1"""
    ns = 70000
    d = synth_blocks(1, 16, seed=21)[0]
    d["code_phase"] = [0.0, 1.0, 1022.0, 1022.999999, 511.5, 0.25, 1022.5, 33.0, 0.0, 1000.0, 7.75, 1.5, 2.0, 3.0, 4.0, 5.0]
    d["carr_phase"] = [0.0, 0.5, 1.0 - 2.0 ** -53, 1.0 / 512, 255.0 / 512, 0.75, 0.25, 2.0 ** -40, 0.0, 0.999, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7]
    fs = 4092000.0
    d["f_carr"] = [0.0, 0.0, fs / 512, -fs / 512, fs / 1024, -fs / 4096, 5000.0, -5000.0, 12345.678, -9876.5, 0.001, -0.001, 2500.0, -2500.0, 100.0, -100.0]
    d["f_code"] = 1.023e6 + d["f_carr"] / 1540.0
    d["f_code"][:2] = 1.023e6
    d["icode"] = [19, 0, 19, 19, 10, 19, 19, 0, 19, 19, 5, 6, 7, 8, 9, 18]
    d["ibit"] = [29, 0, 29, 28, 15, 29, 29, 0, 29, 29, 1, 2, 3, 4, 5, 6]
    d["iword"] = np.arange(16) * 3
    q, _ = gpsiq.quantize(d, fs, ns)
    res = Resident(orc, q[None, :], ns)
    sweep = Sweep()
    for stage in STAGES:
        for ss in (SC08, SC16):
            for j in range(len(MULTS) + 1 if stage != NOISE else len(SIGMAS[NOISE])):      # 6: every clamp and sigma with two multipliers
                st = stage_settings(stage, ss, j, j, j, next_block=40)
                check(ctx, res, ss, variant, st, sc.kernel_of(stage, ss, 16, variant, True), (variant, stage, ss, st))
                sweep.add(stage, ss, st, True)
    sweep.assert_whole((True,))


# ---- either side of each core bound with 4 and 8 channels -----------------------------------------------------------------------------

BOUND_SIGMA, BOUND_SEED = 1000.0, 0           # BOUND_SEED: see extreme_set()


def extreme_set(n, total, nsamp):
    """n channels that differ in nothing but their gain, on a carrier that stands still at phase 0, where the cosine table has its
    peak: every sample's I is +-sum of the (int)(250 g).  The amplitudes are `total` spread over the channels (they differ by one at
    most)."""
    q, _ = gpsiq.quantize_blocks(synth_blocks(2, n, seed=77), 2.6e6, nsamp)
    for f in q.dtype.names:
        q[f][:, 1:] = q[f][:, :1]
    q["carr_phase"], q["carr_step"] = 0, 0
    amp = total // n + (np.arange(n) < total % n)
    q["gain"] = (amp + 0.5) / 250.0
    assert int(np.trunc(250.0 * q["gain"][0]).sum()) == total
    return q


@pytest.mark.parametrize("variant", ["tile", "seg", "segh"])
@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("over", [0, 1])
def test_noise_int16_either_side_of_the_bound(ctx, orc, variant, n, over):
    """n * (int)(250 g) + max |z| = 32767: the plain-add core, whose slot 0 carries the +0x8000 bias (4 and 8 slots: few terms above
    it); 32768: the packed core.  The seed is one for which a sample with I = +-sum draws zI = +-max |z| with the same sign, so the
    extreme sum is reached: the reference says so."""
    nsamp = sc.RAGGED
    mz = sc.max_z(BOUND_SIGMA)
    total = 32767 + over - mz
    res = Resident(orc, extreme_set(n, total, nsamp), nsamp)
    assert np.all(np.abs(res.S[:, 0::2].astype(np.int64)) == total)
    st = Settings(BOUND_SEED, BOUND_SIGMA, 0, None)
    z = nr.noise(st.seed, st.sigma, st.next_block, 2, nsamp)
    assert np.abs(res.S[:, 0::2].astype(np.int64) + z[:, :, 0]).max() == total + mz, "no sample reaches the extreme sum"
    assert res.cls.max_amplitude + mz == 32767 + over
    check(ctx, res, SC16, variant, st, sc.kernel_of(NOISE, SC16, n, variant, not over), (variant, n, over))


@pytest.mark.parametrize("variant", ["tile", "seg", "segh"])
@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("over", [0, 1])
def test_level_either_side_of_the_bound(ctx, orc, variant, n, over):
    """n * (int)(250 g) = 32767: the int16 plain-add core, S = +-32767 in every sample; 32768: the packed core, where +-32768 both
    wrap to -32768 like the reference's (short) cast.  Both formats, with the noise and alone."""
    nsamp = sc.RAGGED
    res = Resident(orc, extreme_set(n, 32767 + over, nsamp), nsamp)
    i = res.S[:, 0::2]
    assert np.all(i == -32768) if over else ((i == 32767).any() and (i == -32767).any() and np.all(np.abs(i.astype(np.int64)) == 32767))
    for k, stage in enumerate((LEVEL_NOISE, LEVEL)):
        for ss, level in ((SC16, (65536, 32767)), (SC16, (40000, 2047)), (SC08, (200, 127)), (SC08, (250, 127))):
            st = Settings(0x57A6E + k, None if stage == LEVEL else BOUND_SIGMA, 60 + k, level)
            check(ctx, res, ss, variant, st, sc.kernel_of(stage, ss, n, variant, not over), (variant, n, over, stage, ss, level))


@pytest.mark.parametrize("variant", ["tile", "seg", "segh"])
def test_int8_noise_with_the_spill_bits_full(ctx, orc, variant):
    """The int8 plain-add core keeps I in a 12-bit field whose carries spill into bits 16..19, below Q's field; the noise term must
    not carry through them into Q.  They are all ones only while all sixteen slots hold a small negative entry: sixteen channels
    that differ in nothing but their gain make that every sample with -4096 <= I < 0, which a random set almost never reaches."""
    nsamp = sc.RAGGED
    q, _ = gpsiq.quantize_blocks(synth_blocks(2, 16, seed=78), 2.6e6, nsamp)
    for f in q.dtype.names:
        q[f][:, 1:] = q[f][:, :1]
    q["gain"] = (0.4 + 0.04 * np.arange(16))
    res = Resident(orc, q, nsamp)
    i = res.S[:, 0::2]
    assert np.mean((i < 0) & (i >= -4096)) > 0.25 and res.cls.max_amplitude < 4096
    for k, ss in enumerate((SC08, SC16)):
        st = Settings(0x5B111 + k, 900.0, 31 + k, None)
        check(ctx, res, ss, variant, st, sc.kernel_of(NOISE, ss, 16, variant, True), (variant, ss))


# ---- the child process of test_cases_that_need_their_own_process ---------------------------------------------------------------------

def child(env):
    import torch
    assert torch.cuda.is_available()
    ctx, orc = gpsiq.Context(0), _oracle.load_oracle()
    cases = [c for c in sc.CASES if c.env == env]
    for c in cases:
        run_case(ctx, orc, c)
        print("ok", c.name, flush=True)
    ctx.close()
    print(f"all {len(cases)} ok")


if __name__ == "__main__":
    child(sys.argv[1])
