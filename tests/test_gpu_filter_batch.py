"""gpsiq_generate_batch_filtered on the MI355X: byte for byte and count for count tests/_filter_ref.py's filter (no head, phase 0) of what
ONE gpsiq_generate_batch over the whole timeline writes on a second context -- 7 blocks of 4 096 samples, 4 channels, noise and level
on -- in pieces of 1 and 3 blocks and whole, in both NCO models, int8 to int8 and int16 to int16, decimated by 1 and by 4; the carrier
phases handed out, a second call that continues the first, the refusals, and a used context called again with a larger shape.
Run with -m gpu."""
import numpy as np
import pytest

import _filter_ref as fr
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

GUARD = 0x7F
TAIL = 64
FS, NB, NSAMP, NC = 10.4e6, 7, 4096, 4
TAPS = gpsiq.filter_design(FS, 1.2e6, 65, 14)


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


def reference(b, d, nsamp, ss, taps, shift, decim, carr):
    """(filter_ref of ONE generate_batch over the whole timeline as [nblocks][2 * nsamp / decim], its count)"""
    want = b.generate_batch(d, nsamp, FS, ss, carr_out=carr)
    out, clipped = fr.filter_ref(want.reshape(-1, 2), None, taps, shift, decim, 0, ss)
    return out.reshape(len(d), -1), clipped


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE], ids=["fixed", "reference"])
@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
@pytest.mark.parametrize("decim", [1, 4])
def test_batch_filtered_is_the_filter_of_one_batch_call(mode, ss, decim, monkeypatch):
    import torch
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        settings(a, mode, ss)
        settings(b, mode, ss)
        d1, d2 = descriptors(800 + ss), descriptors(900 + ss)
        carr_a, carr_b = np.zeros(NC), np.zeros(NC)
        # shift 12: a gain of 4, so that the clamp fires on a levelled stream and the count is not trivially 0
        want, wc = reference(b, d1, NSAMP, ss, TAPS, 12, decim, carr_b)
        assert wc > 0
        rlen = 2 * (NSAMP // decim) * ss
        stride = rlen + 12
        for piece, pieces in (("1", 7), ("3", 3), (None, 1)):
            if piece is None:
                monkeypatch.delenv("GPSIQ_FILTER_PIECE_BLOCKS")
            else:
                monkeypatch.setenv("GPSIQ_FILTER_PIECE_BLOCKS", piece)
            settings(a, mode, ss)                                        # the noise block counter back to 5
            host = np.full(NB * stride + TAIL, GUARD, dtype=np.uint8)
            _, clipped = a.generate_batch_filtered(d1, NSAMP, FS, ss, TAPS, 12, decim, ss, host_ptr=host.ctypes.data, block_stride=stride, carr_out=carr_a)
            assert a.filter_last_plan()[3] == pieces
            body = host[:NB * stride].reshape(NB, stride)
            got = np.ascontiguousarray(body[:, :rlen]).view(want.dtype)
            assert np.array_equal(got, want), (piece, np.argwhere(got != want)[:4])
            assert (body[:, rlen:] == GUARD).all() and (host[NB * stride:] == GUARD).all()
            assert clipped == wc and carr_a.tobytes() == carr_b.tobytes()
        # call 2 continues call 1 (the slots that keep their satellite take the phase handed out), into page-locked memory; its history
        # is zeros again
        monkeypatch.setenv("GPSIQ_FILTER_PIECE_BLOCKS", "3")
        keep = d2["prn"][0] == d1["prn"][-1]
        d2["carr_phase"][0, keep] = carr_a[keep]
        pinned = torch.full((NB * rlen + TAIL,), GUARD, dtype=torch.uint8).pin_memory()
        _, clipped = a.generate_batch_filtered(d2, NSAMP, FS, ss, TAPS, 12, decim, ss, host_ptr=pinned.data_ptr(), carr_out=carr_a)
        want2, wc2 = reference(b, d2, NSAMP, ss, TAPS, 12, decim, carr_b)
        got2 = pinned.numpy()
        assert np.array_equal(got2[:NB * rlen].view(want2.dtype).reshape(NB, -1), want2) and (got2[NB * rlen:] == GUARD).all()
        assert clipped == wc2 and carr_a.tobytes() == carr_b.tobytes() and not np.array_equal(want2, want)
        assert a.noise_state() == b.noise_state()
    finally:
        a.close()
        b.close()


def test_formats_may_differ_and_a_piece_may_be_shorter_than_the_history(monkeypatch):
    """int16 rendered, int8 delivered; 257 taps over blocks of 64 samples in pieces of 1 and 2 blocks: the history of a piece reaches
    back over four and more pieces, inside the staging"""
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        nb, nsamp = 11, 64
        taps = gpsiq.filter_design(FS, 1.0e6, 257, 14)
        d = descriptors(950, nb)
        for c in (a, b):
            settings(c, NCO_FIXED, SC16)
        want = b.generate_batch(d, nsamp, FS, SC16)
        out, wc = fr.filter_ref(want.reshape(-1, 2), None, taps, 20, 2, 0, SC08)
        for piece in ("1", "2"):
            monkeypatch.setenv("GPSIQ_FILTER_PIECE_BLOCKS", piece)
            settings(a, NCO_FIXED, SC16)
            got, clipped = a.generate_batch_filtered(d, nsamp, FS, SC16, taps, 20, 2, SC08)
            assert got.dtype == np.int8 and np.array_equal(got, out.reshape(nb, -1)) and clipped == wc
    finally:
        a.close()
        b.close()


def test_refusals_and_a_used_context_called_again_with_a_larger_shape(monkeypatch):
    import torch
    monkeypatch.delenv("GPSIQ_FILTER_PIECE_BLOCKS", raising=False)
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        d = descriptors(1000)
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_filtered(d, NSAMP, FS, SC08, TAPS, 14, 3, SC08)             # 4 096 % 3 != 0
        assert e.value.code == -1 and "multiple" in str(e.value)
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_filtered(d, NSAMP, FS, SC08, np.array([32767, 32767, 2], np.int16), 14, 4, SC08)
        assert e.value.code == -2
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_filtered(d, NSAMP, FS, SC08, TAPS, 14, 4, SC08, host_ptr=np.zeros(8, np.uint8).ctypes.data, block_stride=16)
        assert e.value.code == -1                                                       # a stride below a row
        # descriptors in device memory: the pieces' first rows are rewritten on the host
        dev = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
        out = np.zeros(NB * 2 * NSAMP, np.uint8)
        clipped = gpsiq.C.c_uint64(0)
        taps = np.ascontiguousarray(TAPS)
        rc = gpsiq._generate_batch_filtered(a._h, dev.data_ptr(), NB, NC, NSAMP, FS, SC08, gpsiq._p(taps), len(taps), 14, 1, SC08, gpsiq._p(out), 2 * NSAMP,
                                            gpsiq.C.byref(clipped), None)
        assert rc == -1
        # a small call, then the same context with more blocks, more samples, more taps and wider elements: grow-only buffers
        for c in (a, b):
            settings(c, NCO_FIXED, SC08)
        got, clipped = a.generate_batch_filtered(d[:2], 512, FS, SC08, TAPS[16:49], 12, 1, SC08)
        want = b.generate_batch(d[:2], 512, FS, SC08)
        ref, wc = fr.filter_ref(want.reshape(-1, 2), None, TAPS[16:49], 12, 1, 0, SC08)
        assert np.array_equal(got, ref.reshape(2, -1)) and clipped == wc
        for c in (a, b):
            settings(c, NCO_FIXED, SC16)
        big = descriptors(1001, 9)
        got, clipped = a.generate_batch_filtered(big, 3 * NSAMP, FS, SC16, TAPS, 14, 4, SC16)
        want = b.generate_batch(big, 3 * NSAMP, FS, SC16)
        ref, wc = fr.filter_ref(want.reshape(-1, 2), None, TAPS, 14, 4, 0, SC16)
        assert np.array_equal(got, ref.reshape(9, -1)) and clipped == wc
        # an empty batch and blocks of no samples
        settings(a, NCO_FIXED, SC08)
        assert a.generate_batch_filtered(d[:0], NSAMP, FS, SC08, TAPS, 14, 4, SC08)[1] == 0
        assert a.generate_batch_filtered(d, 0, FS, SC08, TAPS, 14, 4, SC08)[0].shape == (NB, 0)
    finally:
        a.close()
        b.close()


def test_runahead_filter_flag(tmp_path, monkeypatch):
    """gpsiq_runahead --filter writes the filter of the file the same flags write without it -- every call to the library one span with
    a history of zeros, here the run's three blocks -- at rate / D in the run's own sample size, and prints the clip count"""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    monkeypatch.setenv("GPSIQ_FILTER_PIECE_BLOCKS", "2")        # two pieces
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
    got, text = run("--filter", "500000", "--taps", "33", "--decim", "4")
    want, wc = fr.filter_ref(plain.reshape(-1, 2), None, gpsiq.filter_design(fs, 5e5, 33, 14), 14, 4, 0, SC16)
    assert got.size == nblocks * 2 * (ns // 4) and np.array_equal(got.reshape(-1, 2), want)
    assert f"decimation 4, {wc} elements clipped" in text
