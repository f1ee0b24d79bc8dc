"""gpsiq_acquire on the MI355X: peaks, power grid and correlations equal tests/_acquire_ref.py's restatement of the contract
(include/gpsiq_rows.h, "Acquisition") bit for bit, through the matrix kernels (GPSIQ_ACQUIRE_KERNEL=mfma: acquire_wipe + acquire_mfma
wherever they can serve, also below a full tile) and through the generic kernel (=generic).  The streams are mostly random bytes --
the call is a pure function of (arguments, stream bytes) -- and include the extremes; every case asserts the kernel the planner
names (tests/_acquire_plan.py) and afterwards that the call took it.  Run with -m gpu."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _acquire_plan as ap
import _acquire_ref as ar
import _despread_ref as dr
import _oracle
import gpsiq
from gpsiq.abi import PK4, SC08, SC16, elem_dtype

pytestmark = pytest.mark.gpu

GUARD = 0x7F
KERNELS = ("mfma", "generic")


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


def to_device(stream, base=0, guard=0):
    """elements of one span -> (tensor that owns the memory, device pointer with pointer % 16 == base); `guard` bytes of 0x7f behind,
    and every other byte of the allocation 0x7f as well"""
    import torch
    raw = np.ascontiguousarray(stream).view(np.uint8).ravel()
    buf = torch.full((raw.size + guard + 32,), GUARD, dtype=torch.uint8, device="cuda")
    off = (base - buf.data_ptr()) % 16
    buf[off:off + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf, buf.data_ptr() + off


def random_stream(rng, nsamp, ss):
    info = np.iinfo(elem_dtype(ss))
    x = rng.integers(info.min, info.max + 1, size=2 * nsamp).astype(elem_dtype(ss))
    x[:2], x[-2:] = info.min, info.max                            # the extremes at either end of the span
    return x


def search(ctx, kernel, ptr, nsamp, ss, prns, steps, ndopp, nshift, ncoh, nnoncoh, hop, want="same", corr=True):
    """one call with GPSIQ_ACQUIRE_KERNEL=kernel; asserts the kernel it took"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GPSIQ_ACQUIRE_KERNEL", kernel)
        out = ctx.acquire(nsamp, ss, ptr, prns, *steps, ndopp, nshift, ncoh, nnoncoh, hop, corr=corr)
    took = ctx.acquire_last_plan()
    assert took[0] == (kernel if want == "same" else want), took
    assert out[3] >= 0.0 and (took[1] > 0) == (took[0] == "mfma")
    return out


def same(got, ref):
    for g, r, what in zip(got[:3], ref, ("peaks", "power", "corr")):
        if g is None:
            continue
        assert g.shape == r.shape and g.dtype == r.dtype, what
        assert g.tobytes() == r.tobytes(), (what, np.argwhere(g.view(np.uint8).reshape(-1) != r.view(np.uint8).reshape(-1))[:4] // g.dtype.itemsize)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(stream, steps, reference outputs) of a case of the table, computed once for both kernels"""
    c = [k for k in ap.CASES if k.name == name][0]
    rng = np.random.default_rng(7000 + ap.CASES.index(c))
    nsamp = ap.span_of(c.nshift, c.ncoh, c.nnoncoh, c.hop)
    stream = random_stream(rng, nsamp, c.ss)
    steps = ap.case_steps(c)
    return stream, steps, ar.acquire(_oracle.load_oracle(), stream, c.prns, *steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", ap.CASES, ids=lambda c: c.name)
def test_case_table(ctx, case, kernel):
    c = case
    stream, steps, ref = case_reference(c.name)
    nsamp = len(stream) // 2
    plan = ap.query(nsamp, c.ss, len(c.prns), c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop, kernel)
    assert plan.kernel == kernel
    buf, ptr = to_device(stream, c.base, c.guard)
    assert ptr % 16 == c.base
    first = search(ctx, kernel, ptr, nsamp, c.ss, c.prns, steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop)
    same(first, ref)
    took = ctx.acquire_last_plan()
    assert took[1] == plan.scratch and took[2] == (plan.mx * plan.my * plan.mz if kernel == "mfma" else plan.gx * plan.gy * plan.gz)
    # the call repeated, without the correlations: the same bytes
    again = search(ctx, kernel, ptr, nsamp, c.ss, c.prns, steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop, corr=False)
    assert again[2] is None
    same(again, ref)


def test_the_default_plan_is_the_planner_s(ctx):
    """without the knob: what plan_acquire says for the shape, whichever kernel the library's default is"""
    c = [k for k in ap.CASES if k.name == "rows-d6-ss1"][0]
    stream, steps, ref = case_reference(c.name)
    nsamp = len(stream) // 2
    buf, ptr = to_device(stream)
    got = ctx.acquire(nsamp, c.ss, ptr, c.prns, *steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop, corr=True)
    assert ctx.acquire_last_plan()[0] == ap.query(nsamp, c.ss, len(c.prns), c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop).kernel
    same(got, ref)
    # and a shape below a full tile is generic by default
    small = [k for k in ap.CASES if k.nshift == 17 and k.ndopp >= 2][0]
    stream, steps, ref = case_reference(small.name)
    buf, ptr = to_device(stream)
    same(ctx.acquire(len(stream) // 2, small.ss, ptr, small.prns, *steps, small.ndopp, small.nshift, small.ncoh, small.nnoncoh, small.hop, corr=True), ref)
    assert ctx.acquire_last_plan()[0] == "generic"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("top", [False, True])
def test_extreme_streams(ctx, orc, ss, top, kernel):
    """every element -128 / -32768 (whose negation does not exist in the format), or +127 / +32767"""
    info = np.iinfo(elem_dtype(ss))
    nshift, ncoh, nn, hop, ndopp, prns = 260, 192, 2, 100, 3, (6, 25)
    nsamp = ap.span_of(nshift, ncoh, nn, hop)
    stream = np.full(2 * nsamp, info.max if top else info.min, dtype=elem_dtype(ss))
    steps = ar.steps(2.6e6, -700.0, 700.0)
    buf, ptr = to_device(stream, 4, 16)
    same(search(ctx, kernel, ptr, nsamp, ss, prns, steps, ndopp, nshift, ncoh, nn, hop), ar.acquire(orc, stream, prns, *steps, ndopp, nshift, ncoh, nn, hop))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["p100-int16", "p64-int8", "p16-int16"])
def test_the_lowest_shift_on_a_tie(ctx, name, kernel):
    """a periodic stream searched with carr_step0 = 0: in bin 0 the peak of either satellite is reached at 7, 5 and 16 shifts with
    exactly equal power, a period apart, the first of them past shift 0 (tests/test_stage_contract_cases.py holds that structure on
    the restatement); the peak reported is the lowest.  A reduction that keeps a later lane, tile or iteration fails here."""
    import _contract_cases as cc
    t, stream, ref = cc.tie_reference(name)
    buf, ptr = to_device(stream, 4, 16)
    got = search(ctx, kernel, ptr, len(stream) // 2, t.ss, t.prns, cc.TIE_STEPS, t.ndopp, t.nshift, t.ncoh, t.nnoncoh, t.hop)
    assert [int(s) for s in got[0]["shift"][:, 0]] == [int(s) for s in ref[0]["shift"][:, 0]]
    same(got, ref)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ss", [SC08, SC16])
def test_an_all_zero_stream(ctx, orc, ss, kernel):
    """every power is 0.0 and every peak is at shift 0"""
    nshift, ncoh, nn, hop, ndopp, prns = 300, 128, 2, 150, 2, (4, 21)
    nsamp = ap.span_of(nshift, ncoh, nn, hop)
    stream = np.zeros(2 * nsamp, dtype=elem_dtype(ss))
    steps = ar.steps(2.6e6, 0.0, 500.0)
    buf, ptr = to_device(stream, 8, 16)
    got = search(ctx, kernel, ptr, nsamp, ss, prns, steps, ndopp, nshift, ncoh, nn, hop)
    assert not got[0]["shift"].any() and got[0]["power"].tobytes() == bytes(8 * len(prns) * ndopp) and got[1].tobytes() == bytes(got[1].nbytes)
    same(got, ar.acquire(orc, stream, prns, *steps, ndopp, nshift, ncoh, nn, hop))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ss,ncoh", [(SC16, 320), (SC08, 3072)])
def test_a_coherent_stream_at_full_scale(ctx, orc, ss, ncoh, kernel):
    """code times carrier with every element at the extreme of the format that has the replica's sign: at shift 0 of the right
    satellite and bin every term is positive, X reaches what the format allows and X^2 leaves 2^53, so the power's roundings count;
    int8 at the longest coherent length the matrix path takes (its LDS at 49 920 bytes)"""
    info = np.iinfo(elem_dtype(ss))
    nshift, nn, hop, ndopp, prns = 256, 3, ncoh + 40, 2, (13, 20)
    nsamp = ap.span_of(nshift, ncoh, nn, hop)
    code_step, c0, ci = ar.steps(2.6e6, 1500.0, 500.0)
    s, c = orc.tables()
    idx = ar.carrier_index(c0, nsamp)
    ca = np.concatenate([ar.sampled_code(orc, 13, code_step, ncoh), np.ones(hop - ncoh, dtype=np.int64)] * nn + [np.ones(nshift, dtype=np.int64)])[:nsamp]
    stream = np.stack([np.where(ca * c[idx] >= 0, info.max, info.min), np.where(ca * s[idx] >= 0, info.max, info.min)], axis=1).astype(elem_dtype(ss)).ravel()
    ref = ar.acquire(orc, stream, prns, code_step, c0, ci, ndopp, nshift, ncoh, nn, hop)
    assert ref[0]["shift"][0, 0] == 0 and float(ref[2]["i"][0, 0, 0, 0]) ** 2 > 2.0 ** 53 and ref[1][0, 0, 0] > 2.0 ** 54
    assert int(ref[2]["i"][0, 0, 0, 0]) > 0.85 * ncoh * info.max * 318
    buf, ptr = to_device(stream, 8)
    same(search(ctx, kernel, ptr, nsamp, ss, prns, (code_step, c0, ci), ndopp, nshift, ncoh, nn, hop), ref)


def test_a_long_coherent_length_is_generic_whatever_is_asked(ctx, orc):
    """ncoh 3136: the code copies would not fit the LDS, so GPSIQ_ACQUIRE_KERNEL=mfma gets the generic kernel -- and the right answer"""
    rng = np.random.default_rng(99)
    nshift, ncoh, ndopp, prns = 256, 3136, 2, (2,)
    nsamp = ap.span_of(nshift, ncoh, 1, ncoh)
    stream = random_stream(rng, nsamp, SC08)
    steps = ar.steps(2.6e6, -250.0, 500.0)
    buf, ptr = to_device(stream)
    same(search(ctx, "mfma", ptr, nsamp, SC08, prns, steps, ndopp, nshift, ncoh, 1, ncoh, want="generic"), ar.acquire(orc, stream, prns, *steps, ndopp, nshift, ncoh))


def test_a_page_locked_host_source(ctx, orc):
    """src may be page-locked host memory of gpsiq_host_alloc, read by the device in place (what gpsiq_runahead --acquire does):
    the same bytes as from device memory, through both kernels, with 0x7f behind the span"""
    import ctypes as C
    c = [k for k in ap.CASES if k.name == "negative"][0]
    stream, steps, ref = case_reference(c.name)
    raw = np.ascontiguousarray(stream).view(np.uint8).ravel()
    host = gpsiq._host_alloc(raw.size + 4 + 4096)
    assert host
    try:
        C.memset(host, GUARD, raw.size + 4 + 4096)
        C.memmove(host + 4, raw.ctypes.data, raw.size)
        for kernel in KERNELS:
            same(search(ctx, kernel, host + 4, len(stream) // 2, c.ss, c.prns, steps, c.ndopp, c.nshift, c.ncoh, c.nnoncoh, c.hop), ref)
    finally:
        gpsiq._host_free(host)


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_a_rendered_block_is_searched_blind(ctx, orc):
    """the CPU test's closed loop (tests/test_acquire_ref.py) on the device: gpsiq_launch renders the block with the noise on and
    gpsiq_acquire, told nothing, finds both satellites -- the integers and powers of the CPU reference through both kernels, so the
    threshold measured there needs no second measurement.  Then the same block levelled to 4 bits, packed, unpacked and searched,
    held to the restatement over the unpacked bytes."""
    import torch
    from test_acquire_ref import THRESHOLD, loop_reference
    L, S = dr.LOOP, ar.SEARCH
    d, ref_stream, steps, ref_peaks, ref_power, ref_corr = loop_reference()
    q, _ = gpsiq.quantize_blocks(ar.loop_descriptors(), L["fs"], L["nsamp"])
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], L["fs"])
    ns = L["nsamp"]
    buf = torch.empty(4 * ns, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    args = (S["prns"], steps, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
    ctx.set_noise(L["seed"], sigma, 0)
    try:
        ctx.set_descriptors(q)
        ctx.launch(0, 1, ns, SC16, buf.data_ptr(), 4 * ns, stream=s)
        for kernel in KERNELS:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("GPSIQ_ACQUIRE_KERNEL", kernel)
                got = ctx.acquire(ns, SC16, buf.data_ptr(), args[0], *args[1], *args[2:], stream=s, corr=True)
            assert ctx.acquire_last_plan()[0] == kernel
            same(got, (ref_peaks, ref_power, ref_corr))
        assert np.array_equal(buf.cpu().numpy().view(np.int16), ref_stream)
        ratios = [gpsiq.acquire_decide(got[1][p], S["guard"])[2] for p in range(4)]
        assert min(ratios[:2]) > THRESHOLD > max(ratios[2:]), ratios
        # int8 levelled to 4 bits, through the packer and back
        ctx.set_noise(L["seed"], sigma, 0)
        ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms([L["gain"], L["gain"]], sigma), 2.3), 7)
        b8, pk, un = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (2 * ns, ns, 2 * ns))
        ctx.launch(0, 1, ns, SC08, b8.data_ptr(), 2 * ns, stream=s)
        clipped, _ = ctx.pack(1, ns, SC08, b8.data_ptr(), 2 * ns, PK4, pk.data_ptr(), ns, stream=s)
        ctx.unpack(1, ns, PK4, pk.data_ptr(), ns, SC08, un.data_ptr(), 2 * ns, stream=s)
        x4 = un.cpu().numpy().view(np.int8)
        assert clipped == 0 and np.array_equal(x4, b8.cpu().numpy().view(np.int8)) and np.abs(x4).max() == 7
        ref4 = ar.acquire(orc, x4, *args[0:1], *args[1], *args[2:])
        for kernel in KERNELS:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("GPSIQ_ACQUIRE_KERNEL", kernel)
                got4 = ctx.acquire(ns, SC08, un.data_ptr(), args[0], *args[1], *args[2:], stream=s, corr=True)
            same(got4, ref4)
        r4 = [gpsiq.acquire_decide(got4[1][p], S["guard"]) for p in range(4)]
        print("4-bit stream: " + ", ".join(f"PRN {p} bin {r[0]} shift {r[1]} ratio {r[2]:.4f}" for p, r in zip(S["prns"], r4)))
        for p in range(2):                                            # the same cells as at 16 bits, to a sample
            b16, s16, _ = gpsiq.acquire_decide(ref_power[p], S["guard"])
            assert r4[p][0] == b16 and abs(r4[p][1] - s16) <= 1, (r4[p], b16, s16)
    finally:
        ctx.noise_off()
        ctx.level_off()


# gpsiq_runahead --cn0 c puts a channel of gain 1.0 at c dB-Hz, so a rendered satellite of gain g is at c + 20 log10 g dB-Hz (the
# run's gains are path loss times antenna pattern; --acquire prints them).  Measured once on the MI355X at --cn0 45 --level 42, the
# twelve rendered satellites of the fixture, strongest first (C/N0 in dB-Hz, ratio):
#   PRN 16 43.63 3.0630 | 15 41.46 2.5065 | 4 41.33 1.8968 | 7 40.66 2.3642 | 6 39.05 1.0918 | 13 38.05 1.1409 | 17 37.16 1.0483 |
#   3 36.48 1.0795 | 1 34.80 1.0776 | 11 34.78 1.1181 | 5 34.77 1.0354 | 8 34.71 1.0985;  largest ratio of an absent satellite 1.2664
# Four dwells of a millisecond do not reach below some 40 dB-Hz, and between 40.6 and 41.4 dB-Hz it depends on where a satellite's
# Doppler lies in its 500 Hz bin and its code edge between two samples (PRN 4 is missed at 41.33, PRN 7 found at 40.66): no single
# level splits found from missed.  CN0_FOUND and CN0_MISSED are the two sides of that band, set between the measured values
# 41.46 | 41.33 and 40.66 | 39.05.
CN0_FOUND, CN0_MISSED = 41.4, 40.0
RUNAHEAD_MEASURED = {16: 3.0630, 15: 2.5065, 4: 1.8968, 7: 2.3642, 6: 1.0918, 13: 1.1409, 17: 1.0483, 3: 1.0795, 1: 1.0776, 11: 1.1181, 5: 1.0354, 8: 1.0985}
# --cn0 at which every rendered satellite of the fixture is within reach: the weakest lies 10.3 dB below a channel of gain 1.0, so at 55
# it stands at 44.7 dB-Hz, the level of the CPU test's closed loop.  Measured there: smallest rendered ratio 2.6767 (PRN 1), largest
# absent 1.3532 (at 50: 1.5296 | 1.2877, the weakest not yet found; at 60: 3.8818 | 1.2764; at 65: 4.7264 | 1.2189).
RUNAHEAD_ALL = 55


def runahead_acquire(tmp_path, cn0):
    """gpsiq_runahead --cn0 <cn0> --level 42 --acquire on the synthetic RINEX fixture -> ({prn: ratio} of all 32, {prn: C/N0} of the rendered)"""
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    nblocks, nchan, fs = 1, 12, 2.6e6
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))
    r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"), str(nblocks), str(nchan),
                        repr(fs), "1", str(tmp_path / "o.bin"), "--cn0", str(cn0), "--level", "42", "--acquire"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("acquire PRN")]
    assert [int(w[2]) for w in lines] == list(range(1, 33))
    assert all(-5000.0 <= float(w[3]) <= 5000.0 and 0 <= int(w[6]) < 2600 for w in lines)
    ratio = {int(w[2]): float(w[8]) for w in lines}
    cn0s = {int(w[2]): float(cn0) + 20.0 * np.log10(float(w[11])) for w in lines if len(w) > 9 and w[9] == "rendered"}
    for p in sorted(cn0s, key=cn0s.get, reverse=True):
        print(f"PRN {p:2d}: {cn0s[p]:6.2f} dB-Hz, ratio {ratio[p]:.4f}")
    print("largest ratio of a satellite that is not rendered: %.4f" % max(v for p, v in ratio.items() if p not in cn0s))
    assert len(cn0s) == 12
    return ratio, cn0s


def test_runahead_acquire_at_45_dbhz_finds_what_is_within_reach_and_nothing_else(tmp_path):
    """--cn0 45: every rendered satellite above CN0_FOUND is above the threshold of tests/test_acquire_ref.py, none below CN0_MISSED
    is, and no satellite that is not rendered is (no false alarm).  The twelve rendered ratios are pinned as measured (the run is a
    function of its arguments: fixed seed), so a search that lost a dwell or took another hop or ncoh does not pass."""
    from test_acquire_ref import THRESHOLD
    ratio, cn0 = runahead_acquire(tmp_path, 45)
    found = {p for p, v in ratio.items() if v > THRESHOLD}
    assert found <= set(cn0), sorted(found)
    assert {p for p, v in cn0.items() if v > CN0_FOUND} <= found and not found & {p for p, v in cn0.items() if v < CN0_MISSED}, (sorted(found), cn0)
    assert {p: round(ratio[p], 4) for p in cn0} == RUNAHEAD_MEASURED


def test_runahead_acquire_lists_exactly_the_rendered_satellites(tmp_path):
    """with every rendered satellite within reach (--cn0 RUNAHEAD_ALL): the satellites above the threshold ARE the rendered ones"""
    from test_acquire_ref import THRESHOLD
    assert RUNAHEAD_ALL is not None
    ratio, cn0 = runahead_acquire(tmp_path, RUNAHEAD_ALL)
    assert min(cn0.values()) > CN0_FOUND
    assert {p for p, v in ratio.items() if v > THRESHOLD} == set(cn0), {p: ratio[p] for p in cn0}


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_errors(ctx):
    import ctypes as C
    import torch
    ns = 4096
    buf = torch.zeros(4 * ns + 64, dtype=torch.uint8, device="cuda")
    steps = ar.steps(2.6e6, 0.0, 500.0)
    base = dict(nsamp=ns, ss=SC16, ptr=buf.data_ptr(), prn=[1, 2], ndopp=3, nshift=100, ncoh=128, nnoncoh=2, hop=200)

    def call(**kw):
        a = dict(base, **kw)
        return ctx.acquire(a["nsamp"], a["ss"], a["ptr"], a["prn"], *steps, a["ndopp"], a["nshift"], a["ncoh"], a["nnoncoh"], a["hop"])

    call()
    assert ctx.acquire_last_plan()[0] is not None
    for kw, word in [(dict(ss=4), "bad sample size"), (dict(ss=0), "bad sample size"), (dict(nsamp=-1), "negative size"),
                     (dict(ncoh=0), "coherent length"), (dict(ncoh=32), "coherent length"), (dict(ncoh=100), "coherent length"),
                     (dict(ncoh=(1 << 20) + 64, nsamp=2 ** 31 - 1), "coherent length"), (dict(nshift=0), "each at least 1"), (dict(nnoncoh=0), "each at least 1"),
                     (dict(hop=0), "each at least 1"), (dict(ndopp=0), "Doppler bins"), (dict(ndopp=1025), "Doppler bins"), (dict(prn=[]), "satellites"),
                     (dict(prn=[1] * 33), "satellites"), (dict(prn=[1, 0]), "out of range"), (dict(prn=[33]), "out of range"),
                     (dict(nsamp=99 + 200 + 128 - 1), "the search reads 427 samples"), (dict(nshift=ns), "the search reads"),
                     (dict(nnoncoh=2 ** 31 - 1, hop=2 ** 31 - 1), "the search reads"), (dict(ptr=0), "null source"),
                     (dict(ptr=buf.data_ptr() + 2), "not 4-byte aligned")]:
        with pytest.raises(gpsiq.GpsiqError) as e:
            call(**kw)
        assert e.value.code == -1 and word in str(e.value), (kw, str(e.value))
        assert ctx.acquire_last_plan()[0] is None                   # a call that failed leaves no plan behind
    call(nsamp=427)                                                   # the shortest stream the search fits
    # NULL peaks / NULL list, through the C entry itself
    prn = np.array([1, 2], dtype=np.uint8)
    for peaks, lst in ((None, prn.ctypes.data_as(C.c_void_p)), (np.zeros(6, dtype=gpsiq.ACQ_PEAK_DTYPE).ctypes.data_as(C.c_void_p), None)):
        rc = gpsiq._acquire(ctx._h, ns, SC16, C.c_void_p(buf.data_ptr()), None, lst, 2, steps[0], steps[1], steps[2], 3, 100, 128, 2, 200, peaks, None, None, None)
        assert rc == -1 and "null argument" in gpsiq._last_error().decode()
    rc = gpsiq._acquire(None, ns, SC16, C.c_void_p(buf.data_ptr()), None, prn.ctypes.data_as(C.c_void_p), 2, steps[0], steps[1], steps[2], 3, 100, 128, 2, 200,
                        np.zeros(6, dtype=gpsiq.ACQ_PEAK_DTYPE).ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == -1 and "null context" in gpsiq._last_error().decode()
