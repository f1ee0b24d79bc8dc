"""The case table of the stage kernels (tests/_stage_cases.py) reaches every one of them: each case goes through the plan query
(tests/plan_query.cpp on csrc/gpsiq_launch_plan.h, the header the launcher plans with) with the class of its own descriptors, and the
set of kernels reached equals the list below.  Runs anywhere; tests/test_gpu_stage_matrix.py renders the cases on the MI355X."""
import _plan_query as pq
import _stage_cases as sc

# The stage kernels that exist.  Mirrors csrc/gpsiq_kernels.hip: `Slots` = 4, 8, 12, 16 and `tile_fns`, which instantiates, per
# family (Noise, Level) and format, (64 rows, 1 window per row) and (32, 2), each with the packed (false) and the plain-add (true)
# core; and `generic_kernel`, whose two kernels take the noise table and the level as arguments.
KERNELS = {(k, "noise") for k in (
    "synth_tile_noise<1, 4, 64, 1, false>", "synth_tile_noise<1, 8, 64, 1, false>", "synth_tile_noise<1, 12, 64, 1, false>", "synth_tile_noise<1, 16, 64, 1, false>",
    "synth_tile_noise<1, 4, 64, 1, true>", "synth_tile_noise<1, 8, 64, 1, true>", "synth_tile_noise<1, 12, 64, 1, true>", "synth_tile_noise<1, 16, 64, 1, true>",
    "synth_tile_noise<1, 4, 32, 2, false>", "synth_tile_noise<1, 8, 32, 2, false>", "synth_tile_noise<1, 12, 32, 2, false>", "synth_tile_noise<1, 16, 32, 2, false>",
    "synth_tile_noise<1, 4, 32, 2, true>", "synth_tile_noise<1, 8, 32, 2, true>", "synth_tile_noise<1, 12, 32, 2, true>", "synth_tile_noise<1, 16, 32, 2, true>",
    "synth_tile_noise<2, 4, 64, 1, false>", "synth_tile_noise<2, 8, 64, 1, false>", "synth_tile_noise<2, 12, 64, 1, false>", "synth_tile_noise<2, 16, 64, 1, false>",
    "synth_tile_noise<2, 4, 64, 1, true>", "synth_tile_noise<2, 8, 64, 1, true>", "synth_tile_noise<2, 12, 64, 1, true>", "synth_tile_noise<2, 16, 64, 1, true>",
    "synth_tile_noise<2, 4, 32, 2, false>", "synth_tile_noise<2, 8, 32, 2, false>", "synth_tile_noise<2, 12, 32, 2, false>", "synth_tile_noise<2, 16, 32, 2, false>",
    "synth_tile_noise<2, 4, 32, 2, true>", "synth_tile_noise<2, 8, 32, 2, true>", "synth_tile_noise<2, 12, 32, 2, true>", "synth_tile_noise<2, 16, 32, 2, true>",
    "synth_generic<1>", "synth_generic<2>",
)} | {(k, "level") for k in (
    "synth_tile_level<1, 4, 64, 1, false>", "synth_tile_level<1, 8, 64, 1, false>", "synth_tile_level<1, 12, 64, 1, false>", "synth_tile_level<1, 16, 64, 1, false>",
    "synth_tile_level<1, 4, 64, 1, true>", "synth_tile_level<1, 8, 64, 1, true>", "synth_tile_level<1, 12, 64, 1, true>", "synth_tile_level<1, 16, 64, 1, true>",
    "synth_tile_level<1, 4, 32, 2, false>", "synth_tile_level<1, 8, 32, 2, false>", "synth_tile_level<1, 12, 32, 2, false>", "synth_tile_level<1, 16, 32, 2, false>",
    "synth_tile_level<1, 4, 32, 2, true>", "synth_tile_level<1, 8, 32, 2, true>", "synth_tile_level<1, 12, 32, 2, true>", "synth_tile_level<1, 16, 32, 2, true>",
    "synth_tile_level<2, 4, 64, 1, false>", "synth_tile_level<2, 8, 64, 1, false>", "synth_tile_level<2, 12, 64, 1, false>", "synth_tile_level<2, 16, 64, 1, false>",
    "synth_tile_level<2, 4, 64, 1, true>", "synth_tile_level<2, 8, 64, 1, true>", "synth_tile_level<2, 12, 64, 1, true>", "synth_tile_level<2, 16, 64, 1, true>",
    "synth_tile_level<2, 4, 32, 2, false>", "synth_tile_level<2, 8, 32, 2, false>", "synth_tile_level<2, 12, 32, 2, false>", "synth_tile_level<2, 16, 32, 2, false>",
    "synth_tile_level<2, 4, 32, 2, true>", "synth_tile_level<2, 8, 32, 2, true>", "synth_tile_level<2, 12, 32, 2, true>", "synth_tile_level<2, 16, 32, 2, true>",
    "synth_generic<1>", "synth_generic<2>",
)}


def planned(c):
    """the plan of a case's whole launch, from the class of its own descriptors"""
    st = sc.settings(c)
    return (c.variant, c.ss, c.nsamp, c.nblocks, pq.synth_class(sc.descriptors(c)), None if st.sigma is None else sc.max_z(st.sigma),
            st.level is not None, sc.ENVS[c.env])


def test_the_case_table_reaches_every_stage_kernel():
    assert len(KERNELS) == 68
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    plans = pq.query_many([planned(c) for c in sc.CASES])
    for c, p in zip(sc.CASES, plans):
        assert (p.kernel, p.stage) == (sc.kernel_name(c), sc.stage_family(c)), c.name     # the kernel the case was written for
    assert {(p.kernel, p.stage) for p in plans} == KERNELS
    # the level family both with the noise over the signal and alone, per kernel
    for kind in (sc.LEVEL_NOISE, sc.LEVEL):
        assert {(p.kernel, p.stage) for c, p in zip(sc.CASES, plans) if c.stage == kind} == {k for k in KERNELS if k[1] == "level"}
    for fam in ("noise", "level"):
        tiles = [(c, p) for c, p in zip(sc.CASES, plans) if p.stage == fam and p.kernel.startswith("synth_tile")]
        # several chunks per wave, the last one partial, behind them a tail of one-chunk workgroups
        assert any(p.wave_rows > p.rows and p.wave_rows % p.rows != 0 and 0 < p.big_blocks < c.nblocks for c, p in tiles), fam
        assert any(c.nsamp % 64 != 0 for c, p in tiles), fam
    # every environment a case names exists, and only the empty one runs in the test process itself
    assert {c.env for c in sc.CASES} == set(sc.ENVS)


def test_the_plan_query_speaks_like_the_plan_table():
    """one request answered three ways: arguments, a line of standard input, and the pinned table of tests/test_launch_plans.py"""
    from test_launch_plans import EXPECTED
    cls = pq.SynthClass(0, 8, 32768)
    one = pq.query("segh", 1, 260000, 200, cls, max_z=100, level=True, env={})
    assert one == pq.query_many([("segh", 1, 260000, 200, cls, 100, True, {})])[0]
    line = [s for s in EXPECTED.splitlines() if s.startswith("segh ss=1 n=260000 nb=200 act=8 z=100 lv=1 scr=1 fast=1 pol=0 amp=32768 ")]
    assert len(line) == 1 and line[0].split(" -> ")[1].startswith(one.kernel + " grid=%d " % one.grid)
    assert one.kernel == "synth_tile_level<1, 8, 32, 2, false>" and one.stage == "level"
    assert pq.query("seg", 1, 260000, 200, cls, max_z=100, env={"GPSIQ_NO_FAST": "1"}).kernel == "synth_tile_noise<1, 8, 64, 1, false>"
    assert pq.query("rows", 2, 260000, 200, cls, max_z=100, env={}).kernel == "invalid"
    assert pq.query("seg", 2, 0, 200, cls, env={}).kernel == "none"
    assert pq.auto_variant(pq.ROWS_MAX_CODE_STEP) == "seg" and pq.auto_variant(pq.ROWS_MAX_CODE_STEP + 1) == "segh"
    assert pq.auto_variant(pq.HALF_ROWS_MAX_CODE_STEP + 1) == "generic"
