"""gpsiq_generate_batch_resampled on the MI355X: byte for byte, count for count and carrier phase bit for bit gpsiq_resample (no head)
of what ONE gpsiq_generate_batch over the whole timeline writes on a second context -- 7 blocks of 4 096 samples, 4 channels, noise
and level on -- in pieces of 1, 2 and 3 blocks and whole, in both NCO models, at a ratio above and a ratio below 1, from a position
that is not 0; against tests/_resample_ref.py's restatement and against the device call itself; the refusals, a table whose pieces
are shorter than its history, and gpsiq_runahead --resample.  Run with -m gpu."""
import numpy as np
import pytest

import _resample_ref as rr
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

ONE = 1 << 32
GUARD = 0x7F
TAIL = 64
FS, NB, NSAMP, NC = 10.4e6, 7, 4096, 4
L, NTAPS, SHIFT = 7, 16, 12                        # the designed taps have a sum of 2^14: at shift 12 a gain of 4, so that the clamp fires
DOWN, UP = gpsiq.resample_step(2.6e6, 2.048e6), gpsiq.resample_step(2.6e6, 4.092e6, 20000.0)
POS0 = 3 * ONE + (ONE >> 1) + 12345                 # the first output inside block 0, off the grid


def descriptors(seed, nb=NB, nc=NC):
    """a satellite change on a piece edge (block 3 with pieces of 3) and an unused slot"""
    d = synth_blocks(nb, nc, seed=seed)
    d["prn"][3:, 1] = 29
    d["carr_phase"][3:, 1] = 0.3125
    d["prn"][:, 2] = 0
    return d


def settings(c, mode, ss):
    sigma = gpsiq.noise_sigma_for_cn0(50.0, 1.0, FS)
    c.set_nco_mode(mode)
    c.set_noise(77, sigma, 5)
    q = 127 if ss == SC08 else 32767
    c.set_level(gpsiq.level_mult(gpsiq.composite_rms(np.full(3, 0.6), sigma), q / 4.0), q)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE], ids=["fixed", "reference"])
@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
@pytest.mark.parametrize("step", [DOWN, UP], ids=["down", "up"])
def test_batch_resampled_is_the_resampler_of_one_batch_call(mode, ss, step, monkeypatch):
    import torch
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        settings(a, mode, ss)
        settings(b, mode, ss)
        taps = gpsiq.resample_design(step, 0.8, L, NTAPS, 14)
        d = descriptors(800 + ss)
        carr_a, carr_b = np.zeros(NC), np.zeros(NC)
        stream = b.generate_batch(d, NSAMP, FS, ss, carr_out=carr_b).reshape(-1, 2)
        want, wc, wn, _ = rr.resample_ref(stream, None, taps, L, SHIFT, 1, step, POS0, ss)
        assert wc > 0 and wn == gpsiq.resample_span(NB * NSAMP, POS0, step)[0]
        # the device call itself on the same stream
        src = torch.from_numpy(np.ascontiguousarray(stream).view(np.uint8).ravel().copy()).cuda()
        dst = torch.full((2 * wn * ss + TAIL,), GUARD, dtype=torch.uint8, device="cuda")
        n, _, c, _ = b.resample(NB * NSAMP, ss, src.data_ptr(), taps, L, SHIFT, 1, step, POS0, ss, dst.data_ptr())
        assert n == wn and c == wc and np.array_equal(dst.cpu().numpy()[:2 * wn * ss].view(want.dtype).reshape(-1, 2), want)
        for piece, pieces in (("1", 7), ("2", 4), ("3", 3), (None, 1)):
            if piece is None:
                monkeypatch.delenv("GPSIQ_RESAMPLE_PIECE_BLOCKS")
            else:
                monkeypatch.setenv("GPSIQ_RESAMPLE_PIECE_BLOCKS", piece)
            settings(a, mode, ss)                                        # the noise block counter back to 5
            host = np.full(2 * wn * ss + TAIL, GUARD, dtype=np.uint8)
            nout, clipped = a.generate_batch_resampled(d, NSAMP, FS, ss, taps, L, SHIFT, 1, step, POS0, ss, host_ptr=host.ctypes.data, capacity=wn,
                                                       carr_out=carr_a)
            assert a.resample_last_plan()[3] == pieces and nout == wn
            got = host[:2 * wn * ss].view(want.dtype).reshape(-1, 2)
            assert np.array_equal(got, want), (piece, np.argwhere(got != want)[:4])
            assert (host[2 * wn * ss:] == GUARD).all()
            assert clipped == wc and carr_a.tobytes() == carr_b.tobytes()
        assert a.noise_state() == b.noise_state()
        # one sample short of the span is refused before anything is launched: the noise counter stays
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_resampled(d, NSAMP, FS, ss, taps, L, SHIFT, 1, step, POS0, ss, host_ptr=host.ctypes.data, capacity=wn - 1)
        assert e.value.code == -1 and a.noise_state() == b.noise_state() and (host[2 * wn * ss:] == GUARD).all()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kernel", ["generic", "rows"])
def test_formats_may_differ_and_a_piece_may_be_shorter_than_the_history(kernel, monkeypatch):
    """int16 rendered, int8 delivered, page-locked; 64 taps over blocks of 24 samples in pieces of 1 and 2 blocks at eight samples an
    output: the history of a piece reaches back over three pieces inside the staging, and the output count changes from piece to piece"""
    import torch
    monkeypatch.setenv("GPSIQ_RESAMPLE_KERNEL", kernel)
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        nb, nsamp, step = 11, 24, (1 << 35) - 12345
        taps = gpsiq.resample_design(step, 1.0, 6, 64, 14)
        d = descriptors(950, nb)
        for c in (a, b):
            settings(c, NCO_FIXED, SC16)
        stream = b.generate_batch(d, nsamp, FS, SC16).reshape(-1, 2)
        want, wc, wn, _ = rr.resample_ref(stream, None, taps, 6, 20 - 8, 0, step, 5, SC08)
        for piece in ("1", "2"):
            monkeypatch.setenv("GPSIQ_RESAMPLE_PIECE_BLOCKS", piece)
            settings(a, NCO_FIXED, SC16)
            pinned = torch.full((2 * wn + TAIL,), GUARD, dtype=torch.uint8).pin_memory()
            nout, clipped = a.generate_batch_resampled(d, nsamp, FS, SC16, taps, 6, 20 - 8, 0, step, 5, SC08, host_ptr=pinned.data_ptr(), capacity=wn + 9)
            got = pinned.numpy()
            assert nout == wn and clipped == wc and np.array_equal(got[:2 * wn].view(np.int8).reshape(-1, 2), want) and (got[2 * wn:] == GUARD).all()
            assert a.resample_last_plan()[0] == kernel
    finally:
        a.close()
        b.close()


def test_refusals_and_a_used_context_called_again_with_a_larger_shape(monkeypatch):
    import torch
    monkeypatch.delenv("GPSIQ_RESAMPLE_PIECE_BLOCKS", raising=False)
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        d = descriptors(1000)
        taps = gpsiq.resample_design(DOWN, 0.8, L, NTAPS, 14)
        bad = taps.copy()
        bad[L, :3] = [32767, 32767, 2]
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_resampled(d, NSAMP, FS, SC08, bad, L, 14, 1, DOWN, 0, SC08)
        assert e.value.code == -2
        for kw in (dict(step=(1 << 35) + 1), dict(step=(1 << 29) - 1), dict(pos0=1 << 63), dict(shift=17), dict(interp=2), dict(L=9)):
            args = dict(L=L, shift=14, interp=1, step=DOWN, pos0=0)
            args.update(kw)
            with pytest.raises(gpsiq.GpsiqError) as e:
                a.generate_batch_resampled(d, NSAMP, FS, SC08, taps, args["L"], args["shift"], args["interp"], args["step"], args["pos0"], SC08, capacity=1 << 20)
            assert e.value.code == -1, kw
        # descriptors in device memory: the pieces' first rows are rewritten on the host
        dev = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
        out = np.zeros(NB * 2 * NSAMP, np.uint8)
        nout, clipped = gpsiq.C.c_uint64(0), gpsiq.C.c_uint64(0)
        rc = gpsiq._generate_batch_resampled(a._h, dev.data_ptr(), NB, NC, NSAMP, FS, SC08, gpsiq._p(taps), L, NTAPS, 14, 1, DOWN, 0, SC08, gpsiq._p(out),
                                             NB * NSAMP, gpsiq.C.byref(nout), gpsiq.C.byref(clipped), None)
        assert rc == -1
        # a small call, then the same context with more blocks, more samples, more taps and wider elements: grow-only buffers
        for c in (a, b):
            settings(c, NCO_FIXED, SC08)
        small = gpsiq.resample_design(DOWN, 0.8, 3, 8, 14)
        got, clipped = a.generate_batch_resampled(d[:2], 512, FS, SC08, small, 3, 12, 0, DOWN, 0, SC08)
        ref, wc, wn, _ = rr.resample_ref(b.generate_batch(d[:2], 512, FS, SC08).reshape(-1, 2), None, small, 3, 12, 0, DOWN, 0, SC08)
        assert got.shape == (wn, 2) and np.array_equal(got, ref) and clipped == wc
        for c in (a, b):
            settings(c, NCO_FIXED, SC16)
        big = descriptors(1001, 9)
        wide = gpsiq.resample_design(UP, 0.8, 8, 32, 14)
        got, clipped = a.generate_batch_resampled(big, 3 * NSAMP, FS, SC16, wide, 8, 14, 1, UP, ONE - 1, SC16)
        ref, wc, wn, _ = rr.resample_ref(b.generate_batch(big, 3 * NSAMP, FS, SC16).reshape(-1, 2), None, wide, 8, 14, 1, UP, ONE - 1, SC16)
        assert got.shape == (wn, 2) and np.array_equal(got, ref) and clipped == wc
        # an empty batch, blocks of no samples, and a position past the whole timeline
        settings(a, NCO_FIXED, SC08)
        assert a.generate_batch_resampled(d[:0], NSAMP, FS, SC08, taps, L, 14, 1, DOWN, 0, SC08)[0].shape == (0, 2)
        assert a.generate_batch_resampled(d, 0, FS, SC08, taps, L, 14, 1, DOWN, 0, SC08)[0].shape == (0, 2)
        assert a.generate_batch_resampled(d, NSAMP, FS, SC08, taps, L, 14, 1, DOWN, NB * NSAMP * ONE, SC08)[0].shape == (0, 2)
    finally:
        a.close()
        b.close()


def test_runahead_resample_flag(tmp_path, monkeypatch):
    """gpsiq_runahead --resample writes the resampler of the file the same flags write without it -- every call to the library one span
    with a history of zeros, here the run's three blocks -- at the designed taps, and prints the samples written and the clip count"""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    monkeypatch.setenv("GPSIQ_RESAMPLE_PIECE_BLOCKS", "2")      # two pieces
    fs, nblocks, nchan = 2.6e6, 3, 8
    ns = int(np.floor(fs / 10.0 + 0.5))
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))
    flags = ("--cn0", "45", "--seed", "7", "--level", "9000")

    def run(*more):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), "2", out, *flags, *more], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16), r.stdout
    plain, _ = run()
    assert plain.size == nblocks * 2 * ns
    got, text = run("--resample", "2048000,20000")
    step = gpsiq.resample_step(fs, 2.048e6, 20000.0)
    want, wc, wn, _ = rr.resample_ref(plain.reshape(-1, 2), None, gpsiq.resample_design(step, 0.8, 7, 16, 14), 7, 14, 1, step, 0, SC16)
    assert got.size == 2 * wn and np.array_equal(got.reshape(-1, 2), want)
    assert f"step {step} / 2^32, {wn} samples written, {wc} elements clipped" in text
