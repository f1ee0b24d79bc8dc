"""gpsiq_spectrum on the MI355X: every cell of power equals tests/_spectrum_ref.py's restatement of the contract (include/gpsiq_rows.h,
"Spectrum") byte for byte, on both kernels (GPSIQ_SPECTRUM_KERNEL) and on the default path, whose choice is held to the planner's
(tests/spectrum_plan.cpp).  The spans are random full-range elements -- the kernels are pure functions of the stream -- their base is
aligned to 4 bytes and no more, their length is a multiple of nothing, and the samples behind the last segment that is read are
poison (0x7f7f...) the restatement never sees.  The shapes are the smallest at which a kernel can go wrong: 1, 15, 16, 17 and 33
segments (the edges of a 16-column matrix tile), groups of 1 and 3 with segments left over, groups that end inside a tile and inside a
pass, and one span long enough for a workgroup of the matrix kernel to take several passes.  Run with -m gpu."""
import numpy as np
import pytest

import _spectrum_plan as sp
import _spectrum_ref as sr
import gpsiq
from gpsiq.abi import SC08, SC16, WINDOW_HANN, WINDOW_RECT

pytestmark = pytest.mark.gpu

NFFT = [64, 128, 256, 512]
COUNTS = [1, 15, 16, 17, 33]
FORCE = {"generic": sp.GENERIC, "mfma": sp.MFMA, None: sp.AUTO}
TAIL = 5                         # poisoned samples behind the last segment


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """full-range samples of either format every case cuts its span from (computed once, never written)"""
    rng = np.random.default_rng(99)
    p = {ss: sr.full_range(rng, 80000, ss) for ss in (SC08, SC16)}
    for a in p.values():
        a.setflags(write=False)
    return p


def set_kernel(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("GPSIQ_SPECTRUM_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_SPECTRUM_KERNEL", kernel)


def to_device(x, tail=TAIL):
    """x [n, 2] -> (tensor that keeps the memory, pointer 4 bytes past an 8-byte boundary, samples at the pointer: x and `tail` poisoned ones)"""
    import torch
    raw = np.full(4 + x.nbytes + 2 * tail * x.dtype.itemsize + 8, 0x7F, np.uint8)
    raw[4:4 + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).ravel()
    t = torch.from_numpy(raw).cuda()
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr() + 4, len(x) + tail


def expected_name(plan):
    return None if isinstance(plan, sp.Nothing) else sp.KERNELS[plan.kernel]


@pytest.mark.parametrize("kernel", ["generic", "mfma", None], ids=["generic", "mfma", "default"])
@pytest.mark.parametrize("nfft", NFFT)
def test_sweep_of_formats_hops_windows_shifts_counts_and_groups(ctx, pool, monkeypatch, kernel, nfft):
    set_kernel(monkeypatch, kernel)
    cases = []
    for ss in (SC08, SC16):
        for hop in (nfft // 2, nfft):
            for count in COUNTS:
                cases.append((ss, hop, count))
    for i, (ss, hop, count) in enumerate(cases):
        nlive = (count - 1) * hop + nfft                              # the samples the segments cover
        x = pool[ss][i:i + nlive]
        keep, ptr, nsamp = to_device(x)
        assert sr.span(nsamp, nfft, hop, 1)[0] == count                # the poisoned tail is too short for another segment
        for window in (WINDOW_RECT, WINDOW_HANN):
            for navg in (1, 3):
                shifts = {sr.min_shift(ss, nfft, window, navg), sr.min_shift(ss, nfft, window, navg) + 3}
                if sr.fits(ss, nfft, window, navg, 0):
                    shifts.add(0)
                for shift in sorted(shifts):
                    want = sr.spectrum_ref(x, nfft, hop, window, navg, shift)
                    got = ctx.spectrum(nsamp, ss, ptr, nfft, hop, window, navg, shift)
                    assert got.shape == want.shape == (count // navg, nfft) and got.dtype == np.uint64
                    bad = np.argwhere(got != want)
                    assert not len(bad), (ss, hop, count, window, navg, shift, "first differing cell", bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
                    plan = sp.plan(nsamp, ss, nfft, hop, navg, FORCE[kernel]) if (window, shift) == (WINDOW_RECT, min(shifts)) else None
                    if plan is not None:
                        name, grid, run, groups = ctx.spectrum_last_plan()
                        assert name == expected_name(plan) and groups == count // navg
                        if name is not None:
                            assert (grid, run) == (plan.grid, plan.run)
                        if kernel is not None and ss == SC08 and name is not None:
                            assert name == kernel                      # a forced kernel ran: int8 is served by both
        del keep


@pytest.mark.parametrize("nfft,hop", [(64, 32), (256, 256), (512, 256), (512, 512)])
def test_groups_that_end_inside_tiles_and_passes_give_the_same_bytes_on_both_kernels(ctx, pool, monkeypatch, nfft, hop):
    """150 segments: groups of 20 end inside matrix tiles, groups of 50 span tiles and passes, one group of 150 is summed across passes"""
    count = 150
    x = pool[SC08][7:7 + (count - 1) * hop + nfft]
    keep, ptr, nsamp = to_device(x)
    for navg in (20, 50, 150):
        for window in (WINDOW_RECT, WINDOW_HANN):
            shift = sr.min_shift(SC08, nfft, window, navg)
            want = sr.spectrum_ref(x, nfft, hop, window, navg, shift)
            got = {}
            for kernel in ("generic", "mfma"):
                set_kernel(monkeypatch, kernel)
                got[kernel] = ctx.spectrum(nsamp, SC08, ptr, nfft, hop, window, navg, shift)
                assert ctx.spectrum_last_plan()[0] == kernel
                again = ctx.spectrum(nsamp, SC08, ptr, nfft, hop, window, navg, shift)
                assert got[kernel].tobytes() == again.tobytes(), "two calls, different bytes"
            assert np.array_equal(got["generic"], got["mfma"]) and np.array_equal(got["mfma"], want), (navg, window)


def test_a_workgroup_of_the_matrix_kernel_takes_several_passes(ctx, monkeypatch):
    """nfft 64 with half overlap, 300 001 segments: 4 688 passes of 64 segments over 1 563 workgroups of three passes each.  The two
    kernels are compared on every cell, the restatement on the first and the last group."""
    import torch
    nfft, hop, count, navg = 64, 32, 300_001, 1000
    nsamp = (count - 1) * hop + nfft + 3
    torch.manual_seed(5)
    x = torch.randint(-128, 128, (2 * nsamp + 8,), dtype=torch.int8, device="cuda")
    plan = sp.plan(nsamp, SC08, nfft, hop, navg, sp.MFMA)
    assert plan.per == 3 and plan.ngroups == 300
    got = {}
    for kernel in ("generic", "mfma"):
        set_kernel(monkeypatch, kernel)
        got[kernel] = ctx.spectrum(nsamp, SC08, x.data_ptr(), nfft, hop, WINDOW_HANN, navg, 0)
        assert ctx.spectrum_last_plan() == (kernel, plan.grid if kernel == "mfma" else 300 * 16, 64, 300)
    assert np.array_equal(got["generic"], got["mfma"])
    for g in (0, 299):
        lo = g * navg * hop
        part = x[2 * lo:2 * (lo + (navg - 1) * hop + nfft)].cpu().numpy().reshape(-1, 2)
        assert np.array_equal(sr.spectrum_ref(part, nfft, hop, WINDOW_HANN, navg, 0)[0], got["mfma"][g])
    del x
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_full_scale_spans_at_min_shift(ctx, monkeypatch, kernel):
    set_kernel(monkeypatch, kernel)
    for ss, lo in ((SC08, -128), (SC16, -32768)):
        for nfft in (64, 512):
            navg, count = 33, 34
            spans = [np.full(((count - 1) * nfft + nfft, 2), lo, np.int8 if ss == SC08 else np.int16), sr.adversarial(ss, nfft, count, nfft)]
            for x in spans:
                keep, ptr, nsamp = to_device(x)
                for window in (WINDOW_RECT, WINDOW_HANN):
                    shift = sr.min_shift(ss, nfft, window, navg)
                    want = sr.spectrum_ref(x, nfft, nfft, window, navg, shift)
                    got = ctx.spectrum(nsamp, ss, ptr, nfft, nfft, window, navg, shift)
                    assert np.array_equal(got, want), (ss, nfft, window)
                    assert ctx.spectrum_last_plan()[0] == (kernel if ss == SC08 else "generic")
                del keep


def test_refusals(ctx, pool):
    x = pool[SC08][:2000]
    keep, ptr, nsamp = to_device(x)
    ok = dict(nsamp=nsamp, sample_size=SC08, device_ptr=ptr, nfft=64, hop=64, window=WINDOW_HANN, navg=2, shift=0)
    assert ctx.spectrum(**ok).shape == (15, 64)
    bad = [dict(nfft=32), dict(nfft=1024), dict(nfft=96, hop=96), dict(nfft=0, hop=0), dict(hop=16), dict(hop=128), dict(hop=0), dict(window=2), dict(window=-1),
           dict(navg=0), dict(navg=-3), dict(shift=-1), dict(shift=41), dict(nsamp=-1), dict(sample_size=0), dict(sample_size=4), dict(device_ptr=0),
           dict(device_ptr=ptr + 1), dict(device_ptr=ptr + 2)]
    for change in bad:
        with pytest.raises(gpsiq.GpsiqError) as e:
            ctx.spectrum(**{**ok, **change})
        assert e.value.code == -1, change
    # power NULL: below the Python binding
    assert gpsiq._spectrum(ctx._h, nsamp, SC08, ptr, None, 64, 64, 1, 2, 0, None, None, None) == -1
    # one navg past the bound: int8, nfft 512, Hann holds 536 segments at shift 0
    assert ctx.spectrum(nsamp, SC08, ptr, 512, 512, WINDOW_HANN, 536, 0).shape == (0, 512)
    with pytest.raises(gpsiq.GpsiqError) as e:
        ctx.spectrum(nsamp, SC08, ptr, 512, 512, WINDOW_HANN, 537, 0)
    assert e.value.code == -2
    assert ctx.spectrum(nsamp, SC08, ptr, 512, 512, WINDOW_HANN, 537, 1).shape == (0, 512)
    with pytest.raises(gpsiq.GpsiqError) as e:                        # int16, nfft 512, Hann: nothing fits at shift 3
        ctx.spectrum(nsamp // 2, SC16, ptr, 512, 512, WINDOW_HANN, 1, 3)
    assert e.value.code == -2
    del keep


def test_no_whole_group_leaves_power_untouched(ctx, pool):
    x = pool[SC16][:300]
    keep, ptr, nsamp = to_device(x, tail=0)
    for nfft, hop, navg, n in [(512, 512, 1, 300), (64, 64, 5, 300), (64, 32, 1, 63), (64, 64, 1, 0)]:
        out = np.full((4, nfft), 0x5A5A5A5A5A5A5A5A, np.uint64)
        got = ctx.spectrum(n, SC16, ptr, nfft, hop, WINDOW_HANN, navg, 10, out=out)
        assert got.shape == (0, nfft) and (out == 0x5A5A5A5A5A5A5A5A).all()
        assert ctx.spectrum_last_plan()[0] is None and ctx.spectrum_last_plan()[3] == 0
    # and a call with groups writes exactly its groups
    out = np.full((4, 64), 0x5A5A5A5A5A5A5A5A, np.uint64)
    got = ctx.spectrum(300, SC16, ptr, 64, 64, WINDOW_HANN, 2, 10, out=out)
    assert got.shape == (2, 64) and np.array_equal(got, sr.spectrum_ref(x, 64, 64, 1, 2, 10)) and (out[2:] == 0x5A5A5A5A5A5A5A5A).all()
    del keep


def test_defaults_of_the_binding(ctx, pool):
    x = pool[SC08][:64 * 40]
    keep, ptr, nsamp = to_device(x, tail=0)
    got = ctx.spectrum(nsamp, SC08, ptr, 64)                          # hop nfft, Hann, one group of all 40 segments, min_shift
    assert np.array_equal(got, sr.spectrum_ref(x, 64, 64, WINDOW_HANN, 40, sr.min_shift(SC08, 64, 1, 40)))
    assert ctx.spectrum_ms >= 0.0
    del keep


def test_runahead_spectrum_flag(tmp_path):
    """gpsiq_runahead --spectrum 64 writes the file the same flags write without it, every line it prints without the flag, and
    OUT.psd: the first block through gpsiq_spectrum (Hann, half overlap, one group, min_shift) times gpsiq_spectrum_scale, from -fs/2 up"""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    fs, nblocks, nchan, nfft = 2.6e6, 2, 8, 64
    ns = int(np.floor(fs / 10.0 + 0.5))
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))

    def run(*more):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"), str(nblocks), str(nchan),
                            repr(fs), "2", out, "--cn0", "45", "--seed", "7", "--level", "9000", *more], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16), r.stdout
    plain, text0 = run()
    assert not os.path.exists(str(tmp_path / "o.bin.psd"))
    got, text = run("--spectrum", str(nfft))
    assert np.array_equal(got, plain) and all(line in text.splitlines() for line in text0.splitlines())
    block = plain[:2 * ns].reshape(-1, 2)
    navg = sr.span(ns, nfft, nfft // 2, 1)[0]
    shift = sr.min_shift(SC16, nfft, WINDOW_HANN, navg)
    want = sr.spectrum_ref(block, nfft, nfft // 2, WINDOW_HANN, navg, shift)[0].astype(np.float64) * gpsiq.spectrum_scale(nfft, WINDOW_HANN, navg, shift, fs)
    psd = np.loadtxt(str(tmp_path / "o.bin.psd"))
    k = (np.arange(nfft) + nfft // 2) % nfft
    assert psd.shape == (nfft, 2) and np.allclose(psd[:, 0], np.where(k < nfft // 2, k, k - nfft) * fs / nfft, atol=1e-3)
    assert np.allclose(psd[:, 1], want[k], rtol=1e-8, atol=0.0)
    assert f"spectrum: {nfft} bins" in text and f"{navg} segments, shift {shift}" in text
