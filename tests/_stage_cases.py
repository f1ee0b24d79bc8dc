"""The case table of the stage kernels (synth_tile_noise, synth_tile_level, synth_generic with noise / level): one case per
instantiation and more, each at a block length that ends inside a chunk, a row and a wave.  tests/test_stage_cases.py holds the
table against the list of kernels that exist (on the CPU, through tests/_plan_query.py); tests/test_gpu_stage_matrix.py renders every
case and compares every element with the reference composed here (compose()) from the oracle's noiseless sums, tests/_noise_ref.py and
tests/_level_ref.py.  TEST INFRASTRUCTURE."""
import collections

import numpy as np

import _level_ref as lr
import _noise_ref as nr

SC08, SC16 = 1, 2
NOISE, LEVEL_NOISE, LEVEL = "noise", "level+noise", "level"
STAGES = (NOISE, LEVEL_NOISE, LEVEL)

# rate class -> sample rate: "row" (>= 2.08 Msps: a 64-sample row fits a 32-chip window; tile, seg), "half" (1.023 .. 2.08 Msps:
# segh), "low" (below: generic)
FS = {"row": 5.0e6, "half": 1.5e6, "low": 0.8e6}

# The process environments.  The library reads these knobs once per process, so every non-empty one runs in a child process.
# "grid": no drain cost and a set-up cost far beyond any block makes the planner give every block ONE workgroup whose waves run
# several chunks; one tail workgroup's worth of blocks (capped at half of them) is covered by one-chunk workgroups.  At 70 001 samples
# (1094 rows): wave_rows = 137 = 2 chunks of 64 rows + 9 (seg) / 4 chunks of 32 rows + 9 (segh); of 3 blocks the last is the tail.
ENVS = {
    "": {},
    "nofast": {"GPSIQ_NO_FAST": "1"},
    "grid": {"GPSIQ_SEG_DRAIN": "0", "GPSIQ_SEG_SETUP_ROWS": "1000", "GPSIQ_SEG_TAIL_WGS": "1", "GPSIQ_SEG_MAX_WAVE_ROWS": "512"},
}

# 5 whole 4096-sample chunks + 17 rows + 29 samples: with a window per row (tile, seg) wave 5 of the only workgroup ends inside its
# chunk and inside a row and waves 6, 7 have nothing; with a window per half row (segh: 2048-sample chunks) the same happens in wave
# 2 of the second workgroup
RAGGED = 5 * 4096 + 17 * 64 + 29
LONG = 70001

Case = collections.namedtuple("Case", "name stage ss nact rate variant side nsamp nblocks env seed")


def slots_of(nact):
    return 4 if nact <= 4 else 8 if nact <= 8 else 12 if nact <= 12 else 16


def kernel_of(stage, ss, nact, variant, fast):
    """the instantiation behind a launch of `variant` (tile, seg, segh, generic), in the spelling of tests/launch_plans.cpp"""
    if variant == "generic":
        return "synth_generic<%d>" % ss
    fam = "synth_tile_noise" if stage == NOISE else "synth_tile_level"
    rows, h = (32, 2) if variant == "segh" else (64, 1)
    return "%s<%d, %d, %d, %d, %s>" % (fam, ss, slots_of(nact), rows, h, "true" if fast else "false")


def kernel_name(c):
    """the instantiation the case is written for"""
    return kernel_of(c.stage, c.ss, c.nact, "generic" if c.rate == "low" else c.variant, c.side == "fast")


def stage_family(c):
    return "noise" if c.stage == NOISE else "level"


def _table():
    t = []

    def add(stage, ss, nact, rate, variant, side, nsamp=RAGGED, nblocks=2, env=""):
        name = "%s-sc%02d-%dch-%s-%s-%s%s" % (stage, 8 * ss, nact, rate, variant, side, "-" + env if env else "")
        t.append(Case(name, stage, ss, nact, rate, variant, side, nsamp, nblocks, env, 7000 + len(t)))

    # every instantiation of both families: 2 formats x 4 slot counts x 2 window layouts x 2 cores; the level family once with the
    # noise over the signal and once alone (the zero table).  The slot count is filled in the row layouts and one short in segh.
    for stage in STAGES:
        for ss in (SC08, SC16):
            for slots in (4, 8, 12, 16):
                for layout in ("row", "half"):
                    for side in ("fast", "packed"):
                        tile = (slots in (4, 12)) == (stage == NOISE)
                        variant = "segh" if layout == "half" else "tile" if tile else "seg"
                        nact = slots if layout == "row" else slots - 1
                        # the int8 noise kernels keep 12-bit fields and take the plain-add core whatever the gains: the packed one
                        # is reached with GPSIQ_NO_FAST=1 only
                        env = "nofast" if (stage == NOISE and ss == SC08 and side == "packed") else ""
                        add(stage, ss, nact, layout, variant, side, env=env)
    # generic with each stage, both formats (auto: what the library itself picks below 1.023 Msps)
    for stage in STAGES:
        for ss in (SC08, SC16):
            add(stage, ss, 11, "low", "auto" if ss == SC08 else "generic", "fast")
    # several chunks per wave, the last one partial, the block ending inside it, and a tail of one-chunk workgroups
    add(NOISE, SC16, 4, "row", "seg", "fast", LONG, 3, "grid")
    add(NOISE, SC16, 7, "half", "segh", "packed", LONG, 3, "grid")
    add(NOISE, SC08, 12, "row", "seg", "fast", LONG, 3, "grid")
    add(NOISE, SC08, 8, "half", "segh", "fast", LONG, 3, "grid")
    add(LEVEL_NOISE, SC08, 3, "half", "segh", "packed", LONG, 3, "grid")
    add(LEVEL_NOISE, SC16, 12, "row", "seg", "packed", LONG, 3, "grid")
    add(LEVEL_NOISE, SC08, 8, "row", "seg", "fast", LONG, 3, "grid")
    add(LEVEL, SC16, 4, "half", "segh", "fast", LONG, 3, "grid")
    return t


CASES = _table()


def max_z(sigma):
    """max |z| of the noise table at sigma (S_tail[63]): what the planner adds to the amplitude bound"""
    return int(nr.tables(sigma)[1][63])


# ---- what a case renders -------------------------------------------------------------------------------------------------------

Settings = collections.namedtuple("Settings", "seed sigma next_block level")      # sigma None: noise off; level None or (mult, qmax)


def settings(c):
    """noise and level of a case: the level keeps most samples inside the clamp on either side of the amplitude bound (the fuzz of
    tests/test_gpu_stage_matrix.py sweeps mult and qmax)"""
    sigma = None if c.stage == LEVEL else 900.0 if c.stage == NOISE else 1600.0
    level = None
    if c.stage != NOISE:
        level = {(SC08, "fast"): (1300, 127), (SC08, "packed"): (200, 127), (SC16, "fast"): (200001, 32767), (SC16, "packed"): (40000, 32767)}[(c.ss, c.side)]
    return Settings(0xC0FFEE + c.seed, sigma, 1000 + c.seed, level)


def descriptors(c):
    """quantised descriptors [nblocks][16] of a case: nact active channels; gains on the wanted side of the amplitude bound"""
    import gpsiq
    from gpsiq.scenario import synth_blocks
    d = synth_blocks(c.nblocks, 16, seed=c.seed)
    d["prn"][:, c.nact:] = 0
    k = np.arange(16)
    if c.side == "fast":
        d["gain"] = 0.6 + 0.05 * k                                   # sum of (int)(250 g) <= 3900
    else:
        d["gain"] = 34000.0 / c.nact / 250.0 * (1.0 + 0.01 * k)      # sum of (int)(250 g) > 32767 for any nact
    q, _ = gpsiq.quantize_blocks(d, FS[c.rate], c.nsamp)
    return q


def compose(S, z, ss, level):
    """What a launch must store: S the oracle's wrapped int16 sums [nblocks][2 * nsamp], z the noise of the same absolute blocks
    (tests/_noise_ref.py) or None, then the level stage (mult, qmax) or the wrapping int16 / int8 store."""
    if level is not None:
        return lr.level(S, z, level[0], level[1], ss)
    n16 = S if z is None else nr.add_noise16(S, z)
    return n16 if ss == SC16 else (n16 >> 4).astype(np.int8)
