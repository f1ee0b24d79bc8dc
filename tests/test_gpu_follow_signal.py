"""gpsiq_follow on a stream the library rendered itself, on the MI355X: eight 0.1 s blocks at 2.6 Msps, four channels
(tests/_follow_signal.py), rendered with Context.launch into one contiguous device buffer; the satellites are found by Context.acquire
with 250 Hz bins and started with follow_start, so the receiver is told nothing.  Truth is the quantised descriptors through the
closed form, never the follower.  The conditions are those tests/test_follow_ref.py holds the restatement to on the CPU: from epoch
250 on the code within a quarter chip, no carrier cycle slipped, the prompt at 0.7 of what gpsiq_despread measures, every data bit
read.  Then the same stream as levelled int8 at 50 dB-Hz, and a satellite that is not there.  Run with -m gpu."""
import numpy as np
import pytest

import _follow_ref as fr
import _follow_signal as fsg
import _oracle
import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu

SEARCH = dict(f0=-5000.0, df=250.0, ndopp=41, nshift=2600, ncoh=2560, nnoncoh=4, hop=2600, guard=3)
GAINS = (0.25, 18.0, 5.0)               # gpsiq_follow_gains' fll_gain, pll_bn_hz, dll_bn_hz: the defaults of the binding
MAX_EPOCHS = 900
ABSENT_PRN = 20
CN0, SEED, INT8_RMS = 50.0, 0xF0110, 30.0
SEG = 64 * -(-fsg.NSAMP // 64)       # gpsiq_despread: one segment a block (a multiple of 64 that covers it)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sc():
    s = fsg.scenario(_oracle.load_oracle())
    q, _ = gpsiq.quantize_blocks(s.desc, s.fs, s.nsamp)
    assert q.tobytes() == s.q.tobytes()                 # the library's quantiser and the oracle's agree: one truth
    assert ABSENT_PRN not in set(int(p) for p in s.q["prn"].ravel())
    return s


def render_find_follow(ctx, sc, ss, noise):
    """-> (records [nchan + 1][MAX_EPOCHS], nepochs, states, despread sums [nblocks][nchan]): the channels found blind and followed, and
    behind them the absent satellite from an arbitrary start"""
    import torch
    ns, nb, nchan = sc.nsamp, sc.nblocks, sc.q.shape[1]
    stride = 2 * ns * ss
    buf = torch.empty(nb * stride, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    prns = [int(p) for p in sc.q["prn"][0]]
    try:
        if noise:
            sigma = gpsiq.noise_sigma_for_cn0(CN0, 1.0, sc.fs)
            ctx.set_noise(SEED, sigma, 0)
            ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms([1.0] * nchan, sigma), INT8_RMS), 127)
        ctx.set_descriptors(sc.q)
        ctx.launch(0, nb, ns, ss, buf.data_ptr(), stride, stream=s)
        steps = gpsiq.acquire_steps(sc.fs, SEARCH["f0"], SEARCH["df"])
        S = SEARCH
        _, power, _, _ = ctx.acquire(nb * ns, ss, buf.data_ptr(), prns, *steps, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"], stream=s)
        found = [gpsiq.acquire_decide(power[p], S["guard"]) for p in range(nchan)]
        for k, (d, shift, ratio) in enumerate(found):
            print(f"PRN {prns[k]}: bin {d} ({S['f0'] + d * S['df']:+.0f} Hz, truth {float(sc.desc[0, k]['f_carr']):+.1f}), shift {shift}, ratio {ratio:.2f}")
        states = gpsiq.follow_start(prns, [f[1] for f in found], [f[0] for f in found], *steps)
        absent = fr.make_state(ABSENT_PRN, sample=100, code_step=steps[0], carr_step=steps[1] + 24 * steps[2])
        states = np.concatenate([states, np.array([absent], dtype=states.dtype)])
        rec, n, out, ms = ctx.follow(nb * ns, ss, buf.data_ptr(), gpsiq.follow_gains(sc.fs, *GAINS), states, MAX_EPOCHS, stream=s)
        print(f"follow: {list(n)} epochs, {ms:.2f} ms of kernel for {nb * ns / sc.fs:.1f} s of stream")
        sums, sprn, _, _ = ctx.despread(0, nb, ns, ss, buf.data_ptr(), stride, SEG, stream=s, stats=False)
        assert [int(p) for p in sprn[0]] == prns
        return rec, n, out, sums[:, :, 0]
    finally:
        ctx.noise_off()
        ctx.level_off()


@pytest.fixture(scope="module")
def noiseless(ctx, sc):
    return render_find_follow(ctx, sc, SC16, False)


@pytest.fixture(scope="module")
def noisy(ctx, sc):
    return render_find_follow(ctx, sc, SC08, True)


def reference_amplitude(sc, sums, ch):
    """per sample and block: what gpsiq_despread, which knows the replica, measures for the channel"""
    return np.hypot(sums["i"][:, ch].astype(np.float64), sums["q"][:, ch].astype(np.float64)) / sc.nsamp


def prompt_amplitude(rec):
    return np.hypot(rec["ip"].astype(np.float64), rec["qp"].astype(np.float64)) / rec["nsamp"]


@pytest.mark.parametrize("ch", range(4))
def test_noiseless_int16_every_satellite_locks_and_every_bit_is_read(sc, noiseless, ch):
    rec, n, out, sums = noiseless
    assert out[ch]["status"] == fr.SPAN_END and n[ch] > 700
    r = rec[ch, :n[ch]]
    err = fsg.code_errors(sc, ch, r[fsg.LOCKED_FROM:])
    amp, ref = prompt_amplitude(r[fsg.LOCKED_FROM:]), reference_amplitude(sc, sums, ch)[r["sample"][fsg.LOCKED_FROM:] // sc.nsamp]
    print(f"PRN {int(out[ch]['prn'])}: max |code error| {np.abs(err).max():.4f} chip, smallest prompt / reference {float((amp / ref).min()):.3f}, "
          f"final Doppler {int(out[ch]['carr_step']) * sc.fs / 2.0 ** 59:+.2f} Hz (truth {float(sc.desc[-1, ch]['f_carr']):+.2f})")
    fsg.assert_code_locked(sc, ch, r)
    fsg.assert_carrier_never_slipped(sc, ch, r)
    assert np.all(amp >= 0.7 * ref), float((amp / ref).min())
    fsg.assert_bits_read(sc, ch, r, gpsiq.follow_bits)


@pytest.mark.parametrize("ch", range(4))
def test_levelled_int8_at_50_dbhz_the_bits_are_all_right_and_the_code_holds(sc, noisy, ch):
    """the noise is seeded: one fixed fact, not a probability"""
    rec, n, out, sums = noisy
    assert out[ch]["status"] == fr.SPAN_END and n[ch] > 700
    r = rec[ch, :n[ch]]
    print(f"PRN {int(out[ch]['prn'])}: max |code error| {np.abs(fsg.code_errors(sc, ch, r[fsg.LOCKED_FROM:])).max():.4f} chip")
    fsg.assert_code_locked(sc, ch, r)
    fsg.assert_bits_read(sc, ch, r, gpsiq.follow_bits)


@pytest.mark.parametrize("which", ["noiseless", "noisy"])
def test_a_satellite_that_is_not_in_the_stream_is_followed_to_the_end_and_never_looks_locked(sc, noiseless, noisy, which):
    rec, n, out, sums = noiseless if which == "noiseless" else noisy
    assert out[4]["status"] == fr.SPAN_END and n[4] > 700            # the loop runs on noise without leaving its ranges
    amp = prompt_amplitude(rec[4, :n[4]])
    weakest = min(reference_amplitude(sc, sums, ch).min() for ch in range(4))
    print(f"absent PRN {ABSENT_PRN}: largest prompt {amp.max():.2f} against 0.7 x {weakest:.2f}")
    assert np.all(amp < 0.7 * weakest)


def test_the_device_follows_as_the_restatement_does(sc, noiseless):
    """the first satellite's first 150 records are the restatement's over the same rendered bytes (which are the oracle's: the synthesis
    tests hold that), from the same start"""
    orc = _oracle.load_oracle()
    rec, n, out, _ = noiseless
    stream = np.concatenate([orc.block_fixed(sc.q[b], sc.nsamp, SC16) for b in range(2)])
    start = fr.make_state(int(sc.q[0, 0]["prn"]), sample=int(rec[0, 0]["sample"]), code_step=int(rec[0, 0]["code_step"]), carr_step=int(rec[0, 0]["carr_step"]))
    ref = fr.follow(orc, stream, gpsiq.follow_gains(sc.fs, *GAINS), [start], 150)
    assert ref[1][0] == 150 and ref[0][0].tobytes() == rec[0, :150].tobytes()


# ---- the command line -------------------------------------------------------------------------------------------------------------

def test_runahead_follows_every_satellite_it_lists(tmp_path):
    """gpsiq_runahead --cn0 55 --level 42 --acquire --follow 0.6 on the synthetic RINEX fixture, where --acquire lists exactly the twelve
    rendered satellites (tests/test_gpu_acquire.py): with 250 Hz bins it still lists those twelve, and each is followed to the end of
    the 0.6 s (status 1, one epoch a millisecond) with a final Doppler inside the band searched and within 250 Hz of its bin.  What the
    loops do at each satellite's C/N0 is printed (final Doppler, code phase, prompt amplitude, bits): the weakest stand near 45 dB-Hz,
    below what the default gains are tuned for."""
    import os
    import subprocess
    from test_acquire_ref import THRESHOLD
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    nblocks, nchan, fs = 6, 12, 2.6e6
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))
    r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"), str(nblocks), str(nchan),
                        repr(fs), "1", str(tmp_path / "o.bin"), "--cn0", "55", "--level", "42", "--acquire", "--follow", "0.6"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    acq = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("acquire PRN")]
    fol = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("follow PRN")]
    assert [int(w[2]) for w in acq] == list(range(1, 33))
    rendered = {int(w[2]) for w in acq if len(w) > 9 and w[9] == "rendered"}
    listed = {int(w[2]): float(w[3]) for w in acq if float(w[8]) > THRESHOLD}
    assert len(rendered) == 12 and set(listed) == rendered
    assert all(float(w[3]) % 250.0 == 0.0 for w in acq)                               # the search was widened to 250 Hz bins
    assert [int(w[2]) for w in fol] == sorted(listed)
    for w in fol:
        prn, doppler, code, amp, nbits, epochs, status = int(w[2]), float(w[3]), float(w[6]), float(w[9]), int(w[11]), int(w[13]), int(w[15])
        assert status == fr.SPAN_END and 595 <= epochs <= 600, w
        assert abs(doppler - listed[prn]) < 250.0 and 0.0 <= code < 1023.0 and amp > 0.0, w
        assert nbits == (epochs - 250) // 20 or nbits == (epochs - 250) // 20 - 1, w
