"""gpsiq_generate_batch_mixed on the MI355X: byte for byte and count for count Context.mix (and tests/_mix_ref.py's restatement) of what
ONE gpsiq_generate_batch over the whole timeline writes on a second context -- 7 blocks of 4 099 samples, 4 channels, noise and level
on -- in pieces of 1, 2 and 3 blocks and whole, in both NCO models, int8 and int16; the carrier phases handed out bit for bit, a second
call that continues the first at its absolute sample index, the refusals, and the file gpsiq_runahead --tone writes.
Run with -m gpu."""
import numpy as np
import pytest

import _mix_ref as mr
import gpsiq
from gpsiq.abi import MIX_STREAM, MIX_TONE, NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

GUARD = 0x7F
TAIL = 64
FS, NB, NSAMP, NC = 10.4e6, 7, 4099, 4
SHIFT = 6
M0 = (1 << 32) - 3 * NSAMP - 11                     # the index passes 2^32 inside the call
TONES = [mr.Term(MIX_TONE, 9, step=(37 << 50) + 3, gate=(1000, 400, 17)),                  # amplitudes 9 * 250 / 2^6 = 35 and 20 in int8
         mr.Term(MIX_TONE, -5, phase0=1 << 58, step=-(100 << 50), rate=1 << 47, sweep=(4097, 5))]


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


def reference(b, d, nsamp, ss, base_gain, tones, m0, shift, qmax, carr):
    """(Context.mix of ONE generate_batch over the whole timeline as [nblocks][2 * nsamp], its count), held to the restatement"""
    import torch
    plain = b.generate_batch(d, nsamp, FS, ss, carr_out=carr)
    n = len(d) * nsamp
    src = torch.from_numpy(plain.view(np.uint8).ravel().copy()).cuda()
    dst = torch.zeros_like(src)
    terms = [gpsiq.MixTerm.stream(src.data_ptr(), ss, base_gain)] + [t.mixterm() for t in tones]
    clipped, _ = b.mix(n, m0, terms, shift, qmax, ss, dst.data_ptr())
    out = dst.cpu().numpy().view(plain.dtype).reshape(len(d), -1)
    want, wc = mr.mix_ref(n, m0, [mr.Term(MIX_STREAM, base_gain, plain.reshape(-1, 2))] + list(tones), shift, qmax, plain.dtype)
    assert np.array_equal(out.reshape(-1, 2), want) and clipped == wc
    return out, clipped


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE], ids=["fixed", "reference"])
@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
def test_batch_mixed_is_the_mix_of_one_batch_call(mode, ss, monkeypatch):
    import torch
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        settings(a, mode, ss)
        settings(b, mode, ss)
        d1, d2 = descriptors(800 + ss), descriptors(900 + ss)
        carr_a, carr_b = np.zeros(NC), np.zeros(NC)
        qmax = 100 if ss == SC08 else 30000
        scale = 1 if ss == SC08 else 256                                 # the tones against a stream levelled to a quarter of full scale
        tones = [mr.Term(t.kind, t.gain * scale, phase0=t.phase0, step=t.step, rate=t.rate, sweep=t.sweep, gate=t.gate) for t in TONES]
        base = 3 << SHIFT                                                # a gain of 3, so that the clamp fires and the count is not trivially 0
        want, wc = reference(b, d1, NSAMP, ss, base, tones, M0, SHIFT, qmax, carr_b)
        assert wc > 0
        rlen = 2 * NSAMP * ss
        stride = rlen + 12
        mts = [t.mixterm() for t in tones]
        for piece, pieces in (("1", 7), ("2", 4), ("3", 3), (None, 1)):
            if piece is None:
                monkeypatch.delenv("GPSIQ_MIX_PIECE_BLOCKS")
            else:
                monkeypatch.setenv("GPSIQ_MIX_PIECE_BLOCKS", piece)
            settings(a, mode, ss)                                        # the noise block counter back to 5
            host = np.full(NB * stride + TAIL, GUARD, dtype=np.uint8)
            _, clipped = a.generate_batch_mixed(d1, NSAMP, FS, ss, base, mts, SHIFT, qmax, m0=M0, host_ptr=host.ctypes.data, block_stride=stride,
                                                carr_out=carr_a)
            assert a.mix_last_plan()[3] == pieces
            body = host[:NB * stride].reshape(NB, stride)
            got = np.ascontiguousarray(body[:, :rlen]).view(want.dtype)
            assert np.array_equal(got, want), (piece, np.argwhere(got != want)[:4])
            assert (body[:, rlen:] == GUARD).all() and (host[NB * stride:] == GUARD).all()
            assert clipped == wc and carr_a.tobytes() == carr_b.tobytes()
        # call 2 continues call 1 (the slots that keep their satellite take the phase handed out; the index goes on), into page-locked memory
        monkeypatch.setenv("GPSIQ_MIX_PIECE_BLOCKS", "3")
        keep = d2["prn"][0] == d1["prn"][-1]
        d2["carr_phase"][0, keep] = carr_a[keep]
        pinned = torch.full((NB * rlen + TAIL,), GUARD, dtype=torch.uint8).pin_memory()
        _, clipped = a.generate_batch_mixed(d2, NSAMP, FS, ss, base, mts, SHIFT, qmax, m0=M0 + NB * NSAMP, host_ptr=pinned.data_ptr(), carr_out=carr_a)
        want2, wc2 = reference(b, d2, NSAMP, ss, base, tones, M0 + NB * NSAMP, SHIFT, qmax, carr_b)
        got2 = pinned.numpy()
        assert np.array_equal(got2[:NB * rlen].view(want2.dtype).reshape(NB, -1), want2) and (got2[NB * rlen:] == GUARD).all()
        assert clipped == wc2 and carr_a.tobytes() == carr_b.tobytes() and not np.array_equal(want2, want)
        assert a.noise_state() == b.noise_state()
    finally:
        a.close()
        b.close()


def test_no_tones_refusals_and_a_used_context_called_again_with_a_larger_shape(monkeypatch):
    import torch
    monkeypatch.delenv("GPSIQ_MIX_PIECE_BLOCKS", raising=False)
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        d = descriptors(1000)
        tone = gpsiq.MixTerm.tone(100, 1 << 55)
        for bad in (dict(tones=[gpsiq.MixTerm.stream(4096, SC08, 1)]), dict(tones=[tone] * 8), dict(shift=41), dict(qmax=128), dict(qmax=0),
                    dict(tones=[gpsiq.MixTerm.tone(1, 1, gate=(2, 3, 0))]), dict(host_ptr=np.zeros(8, np.uint8).ctypes.data, block_stride=16)):
            kw = dict(tones=[tone], shift=0, qmax=127)
            kw.update(bad)
            with pytest.raises(gpsiq.GpsiqError) as e:
                a.generate_batch_mixed(d, NSAMP, FS, SC08, 1, kw.pop("tones"), kw.pop("shift"), kw.pop("qmax"), **kw)
            assert e.value.code == -1, bad
        # descriptors in device memory: the pieces' first rows are rewritten on the host
        dev = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
        out = np.zeros(NB * 2 * NSAMP, np.uint8)
        clipped = gpsiq.C.c_uint64(0)
        rc = gpsiq._generate_batch_mixed(a._h, dev.data_ptr(), NB, NC, NSAMP, FS, SC08, 1, None, 0, 0, 0, 127, gpsiq._p(out), 2 * NSAMP, gpsiq.C.byref(clipped), None)
        assert rc == -1
        # no tones and a gain of 1: the batch call's own bytes, clamped; then more blocks, more samples and wider elements: grow-only buffers
        for c in (a, b):
            settings(c, NCO_FIXED, SC08)
        got, clipped = a.generate_batch_mixed(d[:2], 512, FS, SC08, 1, [], 0, 127)
        want = b.generate_batch(d[:2], 512, FS, SC08)
        assert np.array_equal(got, np.clip(want, -127, 127)) and clipped == int(np.count_nonzero(want == -128))
        for c in (a, b):
            settings(c, NCO_FIXED, SC16)
        big = descriptors(1001, 9)
        got, clipped = a.generate_batch_mixed(big, 3 * NSAMP, FS, SC16, 2, [tone], 1, 32767, m0=5)
        want, wc = reference(b, big, 3 * NSAMP, SC16, 2, [mr.Term(MIX_TONE, 100, step=1 << 55)], 5, 1, 32767, None)
        assert np.array_equal(got, want) and clipped == wc
        # an empty batch and blocks of no samples
        settings(a, NCO_FIXED, SC08)
        assert a.generate_batch_mixed(d[:0], NSAMP, FS, SC08, 1, [tone], 0, 127)[1] == 0
        assert a.generate_batch_mixed(d, 0, FS, SC08, 1, [tone], 0, 127)[0].shape == (NB, 0)
    finally:
        a.close()
        b.close()


def test_runahead_tone_flag(tmp_path, monkeypatch):
    """gpsiq_runahead --tone writes the mix of the file the same flags write without it with the tones of gpsiq.mix_tone at the gains of
    gpsiq.mix_gain -- J/S against amplitude 250, a satellite of descriptor gain 1 in an unlevelled stream -- at the run's absolute
    sample index, and prints the clip count"""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    monkeypatch.setenv("GPSIQ_MIX_PIECE_BLOCKS", "2")           # two pieces
    fs, nblocks, nchan = 2.6e6, 3, 8
    ns = int(np.floor(fs / 10.0 + 0.5))
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))
    flags = ("--cn0", "45", "--seed", "7")

    def run(*more):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), "2", out, *flags, *more], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16), r.stdout
    plain, _ = run()
    assert plain.size == nblocks * 2 * ns
    got, text = run("--tone", "250000,20", "--tone", "-400000,34,300000,0.0005")
    terms = [mr.Term(MIX_STREAM, 1 << 8, plain.reshape(-1, 2))]
    for (f0, f1, sweep), js in (((2.5e5, None, 0.0), 20.0), ((-4e5, 3e5, 5e-4), 34.0)):
        step, rate, period = gpsiq.mix_tone(fs, f0, f1, sweep)
        terms.append(mr.Term(MIX_TONE, gpsiq.mix_gain(250.0 * 10.0 ** (js / 20.0), MIX_TONE, 8), step=step, rate=rate, sweep=(period, 0)))
    want, wc = mr.mix_ref(nblocks * ns, 0, terms, 8, 32767, np.int16)
    assert np.array_equal(got.reshape(-1, 2), want) and not np.array_equal(got, plain)
    assert f"tones: 2, {wc} elements clipped" in text
