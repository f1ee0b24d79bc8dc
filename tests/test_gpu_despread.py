"""gpsiq_despread on the MI355X: every sum, satellite and stream statistic equals tests/_despread_ref.py's restatement of the
contract (include/gpsiq_rows.h, "Despread") bit for bit.  The streams are mostly random bytes -- the call is a pure function of
(descriptors, stream bytes) -- and include the extremes; every case first asserts the kernel the planner says it takes
(tests/_despread_plan.py) and afterwards that the call took it.  Run with -m gpu."""
import numpy as np
import pytest

import _despread_plan as dp
import _despread_ref as dr
import _noise_ref as nr
import _oracle
import _plan_query as pq
import gpsiq
from gpsiq.abi import QCHAN_DTYPE, SC08, SC16, elem_dtype
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

GUARD = 0x7F


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


def to_device(stream, guard):
    """stream: [nblocks][2 * nsamp] elements -> (device tensor, stride in bytes); `guard` bytes of 0x7f behind every block"""
    import torch
    raw = np.ascontiguousarray(stream).view(np.uint8).reshape(len(stream), -1)
    buf = np.full((len(stream), raw.shape[1] + guard), GUARD, dtype=np.uint8)
    buf[:, :raw.shape[1]] = raw
    return torch.from_numpy(buf).cuda(), buf.shape[1]


def random_stream(rng, nblocks, nsamp, ss):
    info = np.iinfo(elem_dtype(ss))
    x = rng.integers(info.min, info.max + 1, size=(nblocks, 2 * nsamp)).astype(elem_dtype(ss))
    x[:, :2], x[:, -2:] = info.min, info.max                      # the extremes at either end of every block
    return x


def run(ctx, orc, q, block0, nblocks, nsamp, ss, seg_len, stream, guard=0, clip=None, want_plan=None, stats=True):
    """despread blocks [block0, +nblocks) of the resident set q from `stream` (those blocks' elements) and compare everything"""
    clip = (100 if ss == SC08 else 30000) if clip is None else clip
    dev, stride = to_device(stream, guard)
    stride += (-stride) % 4
    if stride != dev.shape[1]:
        dev, stride = to_device(stream, guard + stride - dev.shape[1])
    sums, prn, st, ms = ctx.despread(block0, nblocks, nsamp, ss, dev.data_ptr(), stride, seg_len, clip=clip, stats=stats)
    if want_plan is not None:
        got = ctx.despread_last_plan()
        assert got[0] == want_plan.kernel and got[2:] == (want_plan.grid, want_plan.wave_rows), (got, want_plan)
        assert want_plan.kernel == "generic" or got[1] == want_plan.slots
    ref_sums, ref_prn = dr.despread(orc, q[block0:block0 + nblocks], stream, nsamp, seg_len)
    assert np.array_equal(prn, ref_prn)
    assert sums.shape == ref_sums.shape and np.array_equal(sums, ref_sums), np.argwhere(sums != ref_sums)[:5]
    if stats:
        assert np.array_equal(st, dr.stats(stream, nsamp, clip)), (st, dr.stats(stream, nsamp, clip))
    assert ms >= 0.0
    return sums, prn, st


def case_descriptors(c):
    d = synth_blocks(c.nres, c.nchan, seed=900 + dp.CASES.index(c))
    for b, pat in enumerate(c.active):
        d["prn"][b, [i for i, ch in enumerate(pat) if ch != "x"]] = 0
    return gpsiq.quantize_blocks(d, c.fs, c.nsamp)[0]


@pytest.mark.parametrize("case", dp.CASES, ids=lambda c: c.name)
def test_case_table(ctx, orc, case, monkeypatch):
    c = case
    for k, v in dp.case_env(c).items():
        monkeypatch.setenv(k, v)
    q = case_descriptors(c)
    cls = pq.synth_class(q)
    plan = dp.query(c.nsamp, c.nblocks, c.seg_len, cls, c.force, c.target)
    assert plan.kernel == c.kernel and cls.max_active == dp.case_class(c).max_active, (plan, cls)
    ctx.set_descriptors(q)
    rng = np.random.default_rng(dp.CASES.index(c))
    stream = random_stream(rng, c.nblocks, c.nsamp, c.ss)
    first = run(ctx, orc, q, c.block0, c.nblocks, c.nsamp, c.ss, c.seg_len, stream, c.guard, want_plan=plan)
    # device order: a block's active channels counted from 0; nothing behind them
    for b in range(c.nblocks):
        na = c.active[c.block0 + b].count("x")
        assert np.all(first[1][b, :na] != 0) and np.all(first[1][b, na:] == 0) and not first[0][b, na:].view(np.int64).any()
    # the call repeated: the same answer (every call zeroes what it adds into)
    again = run(ctx, orc, q, c.block0, c.nblocks, c.nsamp, c.ss, c.seg_len, stream, c.guard, want_plan=plan)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


def test_both_kernels_agree(ctx, orc, monkeypatch):
    """one shape, one stream, both kernels: equal to each other (and each to the reference, above)"""
    c = [k for k in dp.CASES if k.name == "both-rows"][0]
    q = case_descriptors(c)
    ctx.set_descriptors(q)
    stream = random_stream(np.random.default_rng(5), c.nblocks, c.nsamp, c.ss)
    dev, stride = to_device(stream, 0)
    out = {}
    for force in (False, True):
        if force:
            monkeypatch.setenv("GPSIQ_DESPREAD_KERNEL", "generic")
        out[force] = ctx.despread(0, c.nblocks, c.nsamp, c.ss, dev.data_ptr(), stride, c.seg_len, clip=1000)
        assert ctx.despread_last_plan()[0] == ("generic" if force else "rows")
    assert all(np.array_equal(a, b) for a, b in zip(out[False][:3], out[True][:3]))


@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("top", [False, True])
def test_extreme_streams_in_one_segment(ctx, orc, ss, top):
    """every element -32768 / -128 (whose negation does not exist in the format), or +32767 / +127, one segment over 70 001 samples"""
    info = np.iinfo(elem_dtype(ss))
    q = gpsiq.quantize_blocks(synth_blocks(1, 16, seed=31 + ss), 2.6e6, dp.LONG)[0]
    ctx.set_descriptors(q)
    stream = np.full((1, 2 * dp.LONG), info.max if top else info.min, dtype=elem_dtype(ss))
    sums, _, st = run(ctx, orc, q, 0, 1, dp.LONG, ss, 1 << 20, stream, guard=64, clip=info.max)
    assert sums.shape[2] == 1 and st["clip_i"][0] == dp.LONG and st["sumsq_i"][0] == dp.LONG * int(stream[0, 0]) ** 2


def coherent_stream(orc, qc, nsamp, ss):
    """the stream that drives one channel's partial sums as far as they go: every element at the extreme of the format that has the
    sign of the replica's, so that every term is positive and near 2 * 32768 * 250 / sqrt(2)"""
    info = np.iinfo(elem_dtype(ss))
    r = dr.replica(orc, qc, nsamp).reshape(1, -1)
    return np.where(r >= 0, info.max, info.min).astype(elem_dtype(ss))


def test_partial_sums_are_widened_in_time(ctx, orc):
    """a stream coherent with channel 0 in one segment of 70 001 samples: its sum passes 2^39, a lane's 32-bit partial would pass
    2^31 after some 190 rows"""
    q = gpsiq.quantize_blocks(synth_blocks(1, 16, seed=35), 2.6e6, dp.LONG)[0]
    ctx.set_descriptors(q)
    for target in (None, 1):                                      # one-chunk waves, then runs of 256 rows
        with pytest.MonkeyPatch.context() as mp:
            if target:
                mp.setenv("GPSIQ_DESPREAD_TARGET_WGS", str(target))
            sums, _, _ = run(ctx, orc, q, 0, 1, dp.LONG, SC16, 1 << 20, coherent_stream(orc, q[0, 0], dp.LONG, SC16), clip=32767)
            assert ctx.despread_last_plan()[3] == (256 if target else 64)
        assert sums["i"][0, 0, 0] > 2 ** 39 and abs(int(sums["q"][0, 0, 0])) < 2 ** 33


def test_a_whole_block_of_260000_samples_and_16_channels(ctx, orc):
    q = gpsiq.quantize_blocks(synth_blocks(1, 16, seed=26), 2.6e6, 260000)[0]
    ctx.set_descriptors(q)
    stream = random_stream(np.random.default_rng(26), 1, 260000, SC16)
    plan = dp.query(260000, 1, 2560, pq.synth_class(q))
    run(ctx, orc, q, 0, 1, 260000, SC16, 2560, stream, want_plan=plan)
    assert plan.kernel == "rows" and plan.slots == 16


def test_one_segment_over_a_2_5_m_sample_block(ctx, orc):
    """2 500 000 samples at 25 Msps in ONE segment, the stream coherent with channel 0 (its sum passes 2^44), then all -32768"""
    n = 2500000
    q = gpsiq.quantize_blocks(synth_blocks(1, 2, seed=250), 25e6, n)[0]
    ctx.set_descriptors(q)
    sums, _, _ = run(ctx, orc, q, 0, 1, n, SC16, 1 << 30, coherent_stream(orc, q[0, 0], n, SC16), clip=32767)
    assert sums.shape == (1, 2, 1) and sums["i"][0, 0, 0] > 2 ** 44
    run(ctx, orc, q, 0, 1, n, SC16, 1 << 30, np.full((1, 2 * n), -32768, dtype=np.int16), clip=32768)


# ---- raw quantised descriptors --------------------------------------------------------------------------------------------------

def fuzz_set(rng, rows, nc):
    """tests/test_gpu_stage_matrix.py's generator: full-range carrier steps (negative ones too), code steps up to the kernel's limit,
    chips next to the period end, unused slots anywhere"""
    max_step = pq.ROWS_MAX_CODE_STEP if rows else (1 << 57) - 1
    nb, nc = int(rng.integers(1, 4)), nc or int(rng.integers(1, 17))
    ns = int(rng.choice([1, 31, 33, 2047, 2049, 4999, 16384, 16385]))
    q = np.zeros((nb, nc), dtype=QCHAN_DTYPE)
    q["prn"] = rng.integers(0, 33, size=(nb, nc))
    q["prn"][rng.random((nb, nc)) < 0.2] = 0
    q["carr_phase"] = rng.integers(0, 1 << 59, size=(nb, nc), dtype=np.uint64)
    q["carr_step"] = rng.integers(-(1 << 58) + 1, 1 << 58, size=(nb, nc))
    q["code_frac"] = rng.integers(0, 1 << 56, size=(nb, nc), dtype=np.uint64)
    q["code_step"] = rng.integers(1, max_step + 1, size=(nb, nc), dtype=np.uint64)
    q["code_step"][0, :] = max_step                                 # the limit itself
    q["chip0"] = rng.integers(0, 1023, size=(nb, nc))
    q["chip0"][:, ::3] = 1022
    q["icode"] = rng.integers(0, 20, size=(nb, nc))
    q["nav_bits"] = rng.integers(0, 1 << 32, size=(nb, nc), dtype=np.uint64).astype(np.uint32)
    q["gain"] = rng.choice([0.0, 1.0, -3.5, 17.25], size=(nb, nc))   # not part of the replica
    return q, ns


@pytest.mark.parametrize("rows", [True, False], ids=["rows", "generic"])
def test_quantised_descriptor_fuzz(ctx, orc, rows):
    rng = np.random.default_rng(4100 + rows)
    slots = set()
    for case, nc in enumerate([None, 4, 7, 12, 16, None, 9, None]):
        q, ns = fuzz_set(rng, rows, nc)
        cls = pq.synth_class(q)
        seg = int(rng.choice([64, 192, 2560, 1 << 20]))
        plan = dp.query(ns, len(q), seg, cls)
        assert plan.kernel == ("rows" if rows else "generic")
        slots.add(plan.slots)
        ctx.set_descriptors(q)
        ss = (SC08, SC16)[case & 1]
        run(ctx, orc, q, 0, len(q), ns, ss, seg, random_stream(rng, len(q), ns, ss), guard=4 * (case % 3), want_plan=plan)
    assert not rows or len(slots) >= 3


@pytest.mark.parametrize("force", [False, True], ids=["rows", "generic"])
def test_boundary_phases(ctx, orc, force, monkeypatch):
    """carr_phase = 2^59 - 1, code_frac = 2^56 - 1, chip0 = 1022, icode = 19, negative and extreme carrier steps"""
    if force:
        monkeypatch.setenv("GPSIQ_DESPREAD_KERNEL", "generic")
    ns = 70000
    q = gpsiq.quantize_blocks(synth_blocks(1, 8, seed=21), 4.092e6, ns)[0]
    q["carr_phase"][0] = [(1 << 59) - 1, 0, (1 << 59) - 1, 1 << 50, (1 << 50) - 1, (1 << 58), 12345, (1 << 59) - 1]
    q["carr_step"][0] = [1, -1, -(1 << 58) + 1, (1 << 58) - 1, 0, -(1 << 50), (1 << 50) + 1, -7]
    q["code_frac"][0] = [(1 << 56) - 1, 0, (1 << 56) - 1, 1, (1 << 55), (1 << 56) - 1, 0, (1 << 56) - 1]
    q["chip0"][0] = [1022, 0, 1022, 1022, 511, 1022, 0, 1022]
    q["icode"][0] = [19, 0, 19, 19, 10, 19, 19, 0]
    ctx.set_descriptors(q)
    plan = dp.query(ns, 1, 2560, pq.synth_class(q), force)
    run(ctx, orc, q, 0, 1, ns, SC16, 2560, random_stream(np.random.default_rng(8), 1, ns, SC16), want_plan=plan)


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_a_rendered_stream_measures_what_was_set(ctx, orc):
    """the CPU test's closed loop (tests/test_despread_ref.py) on the device: gpsiq_launch renders the channel with the noise on,
    gpsiq_despread reads the same stream -- the integers of the CPU reference, the estimate within 4 sigma of 45 dB-Hz, and the
    gain-0 probe leaves the stream what it is without it, byte for byte"""
    import torch
    from test_despread_ref import loop_reference
    L = dr.LOOP
    q, ref_stream, ref_sums, ref_prn = loop_reference()
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    stride = 4 * L["nsamp"]
    buf = torch.empty(L["nblocks"] * stride, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    ctx.set_noise(L["seed"], sigma, 0)
    try:
        ctx.set_descriptors(q)
        ctx.launch(0, L["nblocks"], L["nsamp"], SC16, buf.data_ptr(), stride, stream=s)
        sums, prn, st, _ = ctx.despread(0, L["nblocks"], L["nsamp"], SC16, buf.data_ptr(), stride, L["seg_len"], clip=32767, stream=s)
        with_probe = buf.cpu().numpy().view(np.int16).reshape(L["nblocks"], -1)
        assert np.array_equal(with_probe, ref_stream)
        assert np.array_equal(sums, ref_sums) and np.array_equal(prn, ref_prn)
        cn0, one = gpsiq.cn0_estimate(sums[:, 0], L["seg_len"], L["fs"])
        print(f"set {L['cn0']} dB-Hz, measured {cn0:.4f} dB-Hz, one sigma {one:.4f} dB")
        assert abs(cn0 - L["cn0"]) <= 4 * one
        # without the probe: the same bytes
        q1 = gpsiq.quantize_blocks(dr.loop_descriptors(with_probe=False), L["fs"], L["nsamp"])[0]
        ctx.set_descriptors(q1)
        buf.zero_()
        ctx.launch(0, L["nblocks"], L["nsamp"], SC16, buf.data_ptr(), stride, stream=s)
        ctx.synchronize(s)
        assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(L["nblocks"], -1), with_probe)
        # the same case through int8 with the level at a third of full scale: the statistics are numpy's on the downloaded stream
        ctx.set_descriptors(q)
        mult = gpsiq.level_mult(gpsiq.composite_rms([L["gain"]], sigma), 127 / 3.0)
        ctx.set_level(mult, 127)
        buf8 = torch.empty(L["nblocks"] * 2 * L["nsamp"], dtype=torch.uint8, device="cuda")
        ctx.launch(0, L["nblocks"], L["nsamp"], SC08, buf8.data_ptr(), 2 * L["nsamp"], stream=s)
        sums8, _, st8, _ = ctx.despread(0, L["nblocks"], L["nsamp"], SC08, buf8.data_ptr(), 2 * L["nsamp"], L["seg_len"], clip=127, stream=s)
        x8 = buf8.cpu().numpy().view(np.int8).reshape(L["nblocks"], -1)
        assert np.array_equal(st8, dr.stats(x8, L["nsamp"], 127)) and st8["clip_i"].sum() > 0
        assert np.array_equal(sums8[:4], dr.despread(orc, q[:4], x8[:4], L["nsamp"], L["seg_len"])[0])
        cn8, one8 = gpsiq.cn0_estimate(sums8[:, 0], L["seg_len"], L["fs"])
        print(f"int8, level at a third of full scale: measured {cn8:.4f} dB-Hz, one sigma {one8:.4f} dB, clipped {st8['clip_i'].sum() / st8.size / L['nsamp']:.5f}")
    finally:
        ctx.noise_off()
        ctx.level_off()


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors(ctx):
    import torch
    ns = 4096
    q = gpsiq.quantize_blocks(synth_blocks(2, 4, seed=3), 2.6e6, ns)[0]
    ctx.set_descriptors(q)
    buf = torch.zeros(2 * 4 * ns + 64, dtype=torch.uint8, device="cuda")

    def call(block0=0, nblocks=2, nsamp=ns, ss=SC16, ptr=None, stride=4 * ns, seg=2560):
        return ctx.despread(block0, nblocks, nsamp, ss, buf.data_ptr() if ptr is None else ptr, stride, seg)

    call()
    for kw, code, word in [(dict(seg=0), -1, "segment length"), (dict(seg=100), -1, "segment length"), (dict(seg=32), -1, "segment length"),
                           (dict(block0=1, nblocks=2), -5, "not resident"), (dict(nblocks=3), -5, "not resident"),
                           (dict(ss=4), -1, "bad sample size"), (dict(ss=0), -1, "bad sample size"),
                           (dict(stride=4 * ns - 4), -1, "block stride"), (dict(stride=4 * ns + 2), -1, "block stride"),
                           (dict(ptr=buf.data_ptr() + 2), -1, "not 4-byte aligned"), (dict(nsamp=-1), -1, "negative size")]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == code and word in str(e.value), (kw, str(e.value))
    # NULL sums, through the C entry itself
    import ctypes as C
    prn = np.zeros((2, 4), dtype=np.uint8)
    rc = gpsiq._despread(ctx._h, 0, 2, ns, SC16, C.c_void_p(buf.data_ptr()), 4 * ns, None, 2560, 0, None, prn.ctypes.data_as(C.c_void_p), None, None)
    assert rc == -1 and "null output" in gpsiq._last_error().decode()
    # a context without descriptors
    c2 = gpsiq.Context(0)
    try:
        c2.resident_nchan = 4
        with pytest.raises(gpsiq.GpsiqError) as e:
            c2.despread(0, 1, ns, SC16, buf.data_ptr(), 4 * ns, 2560)
        assert e.value.code == -5
    finally:
        c2.close()
