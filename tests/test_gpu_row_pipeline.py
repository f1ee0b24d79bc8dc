"""The tile kernels' row loop, four rows per trip with the next row's windows read ahead (csrc/gpsiq_tile_body.inc), against the
oracle at the shapes where that loop can go wrong: rows per wave around the unroll and around the chunk, partial final rows, the
remainder rows behind the last whole trip, the read-ahead across a trip boundary and at the end of a chunk, a nav-bit edge and a
code-period wrap in a row whose windows were read ahead.  Both formats, both cores, used and unused slots, segb and segh, and the
noise and level kernels that include the same body.  Bit-exact; every element of every block is compared.

A wave takes whole trips only in a chunk that lies inside the block (otherwise it checks every row against the block end, one row
per trip).  At these block lengths the planner gives every wave one chunk (64 rows; segh 32), so a block of 64 * k samples leaves
the last wave that has rows k mod 64 of them: the lengths below put that wave at 1, 3, 4, 5 and 63 rows and at exactly one chunk,
and every wave before it on the whole-trip path.  A chunk that holds whole trips AND remainder rows needs a wave with more than
one chunk, which the planner only plans for many long blocks or under the GPSIQ_SEG_* knobs; the library reads those once per
process, so these cases run in one child process: this file run as a script.

Every render is a launch on resident descriptors into a 0x5A-filled buffer whose block stride is larger than the block
(tests/test_gpu_stage_matrix.py's run_device): the padding behind each block and the bytes behind the last one must stay 0x5A.
Run with -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [os.path.join(ROOT, "multi-sdr-gps-sim_amd"), os.path.join(ROOT, "tests")]

import _oracle
import _plan_query as pq
import _stage_cases as sc
import gpsiq
from _stage_cases import LEVEL_NOISE, NOISE, Settings
from gpsiq.abi import NCO_FIXED, SC08, SC16
from gpsiq.scenario import synth_blocks
from test_gpu_stage_matrix import Resident, check, run_device

pytestmark = pytest.mark.gpu

FS = 2.6e6
CHUNK = 64                                               # rows of a chunk at a window per row
# one workgroup per block whose waves own ceil(rows / 8) rows each, the last block covered by one-chunk workgroups
GRID_ENV = sc.ENVS["grid"]
GRID_WAVE_ROWS = (69, 70, 71)                            # a chunk, a trip and 1, 2, 3 remainder rows


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


def descriptors(nb, nact, fs, nsamp, seed, packed=False):
    """[nb][16] quantised, nact active; gains on the wanted side of the int16 amplitude bound (tests/_stage_cases.py)"""
    d = synth_blocks(nb, 16, seed=seed)
    d["prn"][:, nact:] = 0
    k = np.arange(16)
    d["gain"] = 34000.0 / nact / 250.0 * (1.0 + 0.01 * k) if packed else 0.6 + 0.05 * k
    return gpsiq.quantize_blocks(d, fs, nsamp)[0]


def plain_kernel(ss, nact, rows=64, h=1, fast=True, waves_both=None):
    name = "synth_tile<%d, %d, %d, %d, %s" % (ss, sc.slots_of(nact), rows, h, "true" if fast else "false")
    return name + (", 8, true>" if waves_both else ">")


def render_plain(ctx, orc, q, nsamp, ss, variant, kernel, launches=None, env=None):
    """resident blocks [block0, block0 + nb) for each launch, every element against oracle.block_fixed; returns the last plan"""
    ctx.set_nco_mode(NCO_FIXED)
    ctx.noise_off()
    ctx.level_off()
    ctx.set_descriptors(q)
    cls = pq.synth_class(q)
    want = [orc.block_fixed(q[b], nsamp, ss) for b in range(q.shape[0])]
    plan = None
    for block0, nb in launches or [(0, q.shape[0])]:
        plan = pq.query(variant, ss, nsamp, nb, cls, env=env)
        assert plan.kernel == kernel, (plan, kernel)
        got = run_device(ctx, nsamp, ss, variant, block0, nb)
        for b in range(nb):
            bad = np.nonzero(got[b] != want[block0 + b])[0]
            assert bad.size == 0, (f"{kernel} nsamp {nsamp} block {block0}+{b}: {bad.size} of {want[block0 + b].size} elements differ, "
                                   f"first at {bad[:8]}: got {got[b][bad[:8]]} want {want[block0 + b][bad[:8]]}")
    return plan


# ---- rows per wave around the unroll and the chunk ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 4, 5, 63, 64, 65, 67])
def test_rows_of_the_last_wave(ctx, orc, k):
    """64 k samples and one fewer, one more: the last wave with rows has k mod 64 of them (64: a whole chunk, on the whole-trip path
    when the block ends with it and on the checked path one sample short), with and without a partial final row.  Three blocks in
    one launch, then one block alone."""
    for nsamp in (CHUNK * k - 1, CHUNK * k, CHUNK * k + 1):
        q = descriptors(3, 16, FS, nsamp, seed=100 + k)
        for ss in (SC08, SC16):
            plan = render_plain(ctx, orc, q, nsamp, ss, "seg", plain_kernel(ss, 16), launches=[(0, 3), (2, 1)])
            assert plan.wave_rows == CHUNK and plan.tiles == 1, plan


# ---- both formats, both cores, unused slots, the both-polarity table ------------------------------------------------------------------

@pytest.mark.parametrize("nact", [16, 5])
@pytest.mark.parametrize("ss,packed", [(SC08, False), (SC16, False), (SC16, True)], ids=["int8", "int16-plain-add", "int16-packed"])
def test_formats_cores_and_unused_slots(ctx, orc, ss, packed, nact):
    """wave 0 a whole chunk (sixteen trips, the last one reading ahead inside the chunk), wave 1 three rows and one sample.
    int16 either side of sum (int)(250 |gain|) <= 32767; 5 channels leave three of eight slots unused"""
    nsamp = CHUNK * 67 + 1
    q = descriptors(2, nact, FS, nsamp, seed=200 + nact + ss, packed=packed)
    amp = pq.synth_class(q).max_amplitude
    assert (amp > 32767) == packed, amp
    for variant in ("seg", "tile"):
        render_plain(ctx, orc, q, nsamp, ss, variant, plain_kernel(ss, nact, fast=not packed))
    if not packed:                                          # segb: sixteen waves, chunks of both_rows(slots) rows
        rows = pq.query("segb", ss, nsamp, 2, pq.synth_class(q)).rows
        render_plain(ctx, orc, q, nsamp, ss, "segb", plain_kernel(ss, nact, rows=rows, waves_both=True))


def test_half_row_windows(ctx, orc):
    """segh at 1.5 Msps: two windows per row, chunks of 32 rows.  Wave 0 a whole chunk (eight trips), wave 1 three rows and one sample"""
    fs, nsamp = 1.5e6, 64 * 35 + 1
    for nact in (16, 5):
        q = descriptors(2, nact, fs, nsamp, seed=300 + nact)
        assert pq.auto_variant(pq.synth_class(q).max_code_step) == "segh"
        for ss in (SC08, SC16):
            render_plain(ctx, orc, q, nsamp, ss, "segh", plain_kernel(ss, nact, rows=32, h=2))


# ---- the kernels that include the same body --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nact", [16, 5])
@pytest.mark.parametrize("stage", [NOISE, LEVEL_NOISE])
@pytest.mark.parametrize("nsamp", [CHUNK * 5 + 1, CHUNK * 69 + 1])
def test_noise_and_level_kernels(ctx, orc, stage, nact, nsamp):
    """noise alone and the level stage over the noise (mult != 0), at five rows and a sample (every row checked) and at a whole chunk,
    five rows and a sample (whole trips in wave 0); against the oracle's sums with tests/_noise_ref.py and tests/_level_ref.py"""
    try:
        res = Resident(orc, descriptors(2, nact, FS, nsamp, seed=400 + nact), nsamp)
        for ss in (SC08, SC16):
            level = None if stage == NOISE else {SC08: (1300, 127), SC16: (200001, 32767)}[ss]
            st = Settings(0xC0FFEE + nsamp, 900.0 if stage == NOISE else 1600.0, 1000 + nact, level)
            check(ctx, res, ss, "seg", st, sc.kernel_of(stage, ss, nact, "seg", True), (stage, ss, nact, nsamp))
    finally:
        ctx.noise_off()
        ctx.level_off()


# ---- a nav-bit edge and a code-period wrap in a row whose windows were read ahead --------------------------------------------------------

def wrap_sample(qc):
    """first sample of the block at which the channel's chip count passes the end of the code period"""
    n = np.arange(1024, dtype=object)
    a = int(qc["chip0"]) + ((int(qc["code_frac"]) + int(qc["code_step"]) * n) >> 56)
    return int(np.argmax(np.array([int(x) >= 1023 for x in a])))


@pytest.mark.parametrize("first_row", [4, 8], ids=["row4", "row8"])
def test_edges_in_the_first_row_behind_a_trip_boundary(ctx, orc, first_row):
    """every channel's code period ends inside row `first_row` of wave 0 (the first row of a trip: its windows were read while the
    trip before it was worked), each at another sample; on the even channels that is the end of a nav bit whose successor differs
    (icode 19, alternating bits), on the odd ones a period wrap inside a bit"""
    nsamp = CHUNK * 67 + 1
    q = descriptors(2, 16, FS, nsamp, seed=500 + first_row).copy()
    chips_per_row = 64 * 1.023e6 / FS
    for c in range(16):
        q["chip0"][:, c] = 1023 - int(first_row * chips_per_row) - 3 - c
        q["icode"][:, c] = 19 if c % 2 == 0 else 5
        q["nav_bits"][:, c] = 0xAAAAAAAA if c % 4 == 0 else 0x55555555
    at = [wrap_sample(q[b, c]) for b in range(2) for c in range(16)]
    assert all(64 * first_row <= n < 64 * (first_row + 1) for n in at) and len(set(at)) > 8, at
    for ss in (SC08, SC16):
        render_plain(ctx, orc, q, nsamp, ss, "seg", plain_kernel(ss, 16))


# ---- whole trips and remainder rows in one chunk: waves of several chunks -----------------------------------------------------------------

def grid_cases(ctx, orc):
    """one workgroup per block, every wave wave_rows = 69, 70, 71 rows: a chunk, then a chunk of one trip and 1, 2, 3 remainder rows
    whose stores follow the trip's immediate offsets.  With the last row whole every wave is on the whole-trip path; 29 samples short,
    the last wave checks its rows.  int8 and int16, 16 channels and 5.  Three blocks: the last one is the tail of one-chunk workgroups"""
    done = 0
    for wr in GRID_WAVE_ROWS:
        for nsamp, ss, nact in ((8 * wr * 64, SC08, 16), (8 * wr * 64 - 29, SC16, 5)):
            q = descriptors(3, nact, FS, nsamp, seed=600 + wr + nact)
            plan = render_plain(ctx, orc, q, nsamp, ss, "seg", plain_kernel(ss, nact), env=os.environ)
            assert plan.wave_rows == wr and plan.tiles == 1 and plan.big_blocks == 2, plan
            done += 1
            print("ok", wr, nsamp, ss, nact, flush=True)
    return done


def test_remainder_rows_behind_a_whole_trip():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **GRID_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"all {len(GRID_WAVE_ROWS) * 2} ok" in r.stdout, (r.returncode, (r.stdout + r.stderr)[-4000:])


if __name__ == "__main__":
    assert {k: os.environ.get(k) for k in GRID_ENV} == GRID_ENV, "the cases need the grid-shape knobs"
    c = gpsiq.Context(0)
    n = grid_cases(c, _oracle.load_oracle())
    c.close()
    print(f"all {n} ok")
