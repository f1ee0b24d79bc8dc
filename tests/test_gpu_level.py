"""The output level stage on the MI355X: every element the kernels store equals the numpy restatement (tests/_level_ref.py) of
include/gpsiq_rows.h's contract -- noise alone and over the signal, both formats, both NCO models, every core and every kernel
that has the stage, however a timeline is split into calls -- and level off leaves everything as it was.  Every block a test renders
is compared.  The noiseless int16 stream S the restatement starts from is the oracle's in the fixed-point model (the library's
level-off render, asserted equal to the oracle block for block); in GPSIQ_NCO_REFERENCE it is the library's level-off render, which
tests/test_gpu_reference_nco.py holds against the reference's loop.  Run with -m gpu.
The list-overflow fall-back of the device-evaluated batch is in tests/test_gpu_level_fallback.py (it needs the test-hook build)."""
import os
import subprocess

import numpy as np
import pytest

import _level_ref as lr
import _noise_ref as nr
import _oracle
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

SEED = 0x1E7E1
QMAX = {SC08: (1, 7, 127), SC16: (2047, 32767)}


@pytest.fixture(scope="module")
def ctxs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    cs = [gpsiq.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def fresh(ctx, mode, seed=None, sigma=0.0, next_block=0, level=None):
    ctx.set_nco_mode(mode)
    if seed is None:
        ctx.noise_off()
    else:
        ctx.set_noise(seed, sigma, next_block)
    if level is None:
        ctx.level_off()
    else:
        ctx.set_level(*level)


def mults_for(rms, qmax):
    """one that puts the rms at a third of the clamp, one below and one above 65536"""
    return sorted({gpsiq.level_mult(rms, qmax / 3.0), 40000, 200001})


def patchy(desc, fs, nb):
    """two channels a hair short of a chip edge at a whole number of samples per chip: GPSIQ_NCO_REFERENCE then has patches"""
    rng = np.random.default_rng(int(fs))
    desc["code_phase"][:, :2] = (rng.integers(0, 1023, (nb, 2)) + 1.0 - 1e-10) % 1023.0
    desc["f_code"][:, :2] = fs / 7


def held_to_oracle(clean, desc, fs, nsamp):
    """fixed-point model: the noiseless stream the restatement starts from is the oracle's, block for block"""
    orc, q = _oracle.load_oracle(), gpsiq.quantize_blocks(desc, fs, nsamp)[0]
    for b in range(desc.shape[0]):
        assert np.array_equal(clean[b], orc.block_fixed(q[b], nsamp, SC16, seq=True)), f"level-off block {b} differs from the oracle"


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("fs,nact", [(0.8e6, 16), (0.8e6, 12), (1.5e6, 16), (1.5e6, 12), (2.6e6, 16), (2.6e6, 12), (10e6, 16), (10e6, 12), (25e6, 16), (25e6, 12)])
def test_noise_over_signal(ctxs, mode, fs, nact):
    """generic (0.8 Msps), segh (1.5) and seg; every block rendered is compared, for every qmax of both formats and three multipliers"""
    nb, nsamp, sigma = 6, int(round(fs / 10)), 1600.0
    desc = synth_blocks(nb, 16, seed=int(fs) % 1000 + mode)
    desc["prn"][:, nact:] = 0
    if mode == NCO_REFERENCE:
        patchy(desc, fs, nb)
        if fs >= 25e6:
            assert len(gpsiq.reference_blocks(desc, fs, nsamp)[1]) > 0
    fresh(ctxs[0], mode)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    if mode == NCO_FIXED:
        held_to_oracle(clean, desc, fs, nsamp)
    z = nr.noise(SEED, sigma, 77, nb, nsamp)
    rms = gpsiq.composite_rms(desc["gain"][0, :nact], sigma)
    for ss in (SC08, SC16):
        for qmax in QMAX[ss]:
            for mult in mults_for(rms, qmax):
                fresh(ctxs[1], mode, SEED, sigma, 77, (mult, qmax))
                got = ctxs[1].generate_batch(desc, nsamp, fs, ss)
                assert np.array_equal(got, lr.level(clean, z, mult, qmax, ss)), f"format {ss} qmax {qmax} mult {mult}"


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_noise_over_signal_through_the_device_evaluated_batch(ctxs, mode, monkeypatch):
    """48 blocks: the batch whose descriptors are quantised / evaluated on the device; all 48 compared"""
    monkeypatch.setenv("GPSIQ_EVAL", "device")
    nb, fs, sigma = 48, 2.6e6, 1600.0
    nsamp = int(round(fs / 10))
    desc = synth_blocks(nb, 16, seed=600 + mode)
    if mode == NCO_REFERENCE:
        patchy(desc, fs, nb)
    fresh(ctxs[0], mode)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    if mode == NCO_FIXED:
        held_to_oracle(clean, desc, fs, nsamp)
    z = nr.noise(SEED, sigma, 77, nb, nsamp)
    rms = gpsiq.composite_rms(desc["gain"][0], sigma)
    for ss, qmax in ((SC08, 127), (SC08, 1), (SC16, 2047)):
        mult = gpsiq.level_mult(rms, qmax / 3.0)
        fresh(ctxs[1], mode, SEED, sigma, 77, (mult, qmax))
        st0 = gpsiq.device_eval_stats()
        got = ctxs[1].generate_batch(desc, nsamp, fs, ss)
        assert gpsiq.device_eval_stats()[0] > st0[0], "the call should have taken the device path"
        assert np.array_equal(got, lr.level(clean, z, mult, qmax, ss)), (ss, qmax)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("fs,sigma", [(0.8e6, 889.0), (1.5e6, 1218.0), (2.6e6, 1603.0), (10e6, 3144.0), (25e6, 15718.0)])
def test_pure_noise(ctxs, mode, fs, sigma):
    """no signal, every kernel (generic, segh, seg); at the last sigma some |A| exceed 32767, which only the level path can
    represent.  Multipliers: the one that puts the rms at a third of the clamp, one below and one above 65536."""
    nb, nsamp = 4, int(round(fs / 10))
    desc = synth_blocks(nb, 16, seed=11)
    desc["gain"] = 0.0
    z = nr.noise(SEED, sigma, 10**9, nb, nsamp)
    if sigma > 10000:
        assert np.mean(np.abs(z) > 32767) > 0.02
    for ss in (SC08, SC16):
        for qmax in QMAX[ss]:
            for mult in mults_for(sigma, qmax):
                fresh(ctxs[0], mode, SEED, sigma, 10**9, (mult, qmax))
                out = ctxs[0].generate_batch(desc, nsamp, fs, ss)
                assert np.array_equal(out, lr.stage(z, mult, qmax).reshape(nb, 2 * nsamp).astype(out.dtype)), (ss, qmax, mult)
                assert ctxs[0].noise_state()[2] == 10**9 + nb


@pytest.mark.parametrize("noise_on", [False, True])
@pytest.mark.parametrize("amp", [2047, 2048, 3000])
def test_both_cores_with_and_without_noise(ctxs, amp, noise_on):
    """16 channels of amplitude amp: 16 * 2047 = 32752 takes the plain-add core, 16 * 2048 the packed one (3000: sums that wrap);
    with the level on the noise does not enter that choice.  noise_on False: the level stage alone."""
    nb, nsamp, fs, sigma = 2, 260000, 2.6e6, 5000.0
    desc = synth_blocks(nb, 16, seed=9)
    desc["gain"] = amp / 250.0 + 1e-9
    assert int(250 * desc["gain"][0, 0]) == amp
    fresh(ctxs[0], NCO_FIXED)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    held_to_oracle(clean, desc, fs, nsamp)
    z = nr.noise(1, sigma, 0, nb, nsamp) if noise_on else None
    for ss, qmax, mult in ((SC08, 127, 300), (SC08, 7, 20), (SC16, 32767, 65536), (SC16, 2047, 70000), (SC16, 32767, 2 ** 24 - 1), (SC08, 1, 1)):
        fresh(ctxs[1], NCO_FIXED, 1 if noise_on else None, sigma, 0, (mult, qmax))
        got = ctxs[1].generate_batch(desc, nsamp, fs, ss)
        assert np.array_equal(got, lr.level(clean, z, mult, qmax, ss)), (ss, qmax, mult)
        if not noise_on and (ss, qmax, mult) == (SC16, 32767, 65536):           # the unit level is the identity, in the kernels too
            assert np.array_equal(got[clean != -32768], clean[clean != -32768]) and np.all(got[clean == -32768] == -32767)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_split_invariance(ctxs, mode, monkeypatch):
    """one batch == block calls == mixed batches == gpsiq_generate_batch_multi == quantised shards == gpsiq_launch"""
    import torch
    nb, nsamp, fs, sigma, ss = 64, 260000, 2.6e6, 1603.0, SC08
    lv = (gpsiq.level_mult(sigma, 42.0), 127)
    desc = synth_blocks(nb, 12, seed=21)
    c = ctxs[0]
    fresh(c, mode, SEED, sigma, 1000, lv)
    whole = c.generate_batch(desc, nsamp, fs, ss)
    fresh(ctxs[1], mode)
    clean = ctxs[1].generate_batch(desc, nsamp, fs, SC16)
    if mode == NCO_FIXED:
        held_to_oracle(clean, desc, fs, nsamp)
    assert np.array_equal(whole, lr.level(clean, nr.noise(SEED, sigma, 1000, nb, nsamp), lv[0], lv[1], ss))

    def continued(b, carr):
        d = desc[b:].copy()
        if carr is not None:
            d["carr_phase"][0] = carr
        return d

    fresh(c, mode, SEED, sigma, 1000, lv)
    carr = None
    for b in range(nb):
        out, carr = c.generate_block(continued(b, carr)[0], nsamp, fs, ss)
        assert np.array_equal(out, whole[b]), f"block call {b}"
    fresh(c, mode, SEED, sigma, 1000, lv)
    b0, carr = 0, None
    for n in (1, 5, 50, 8):
        co = np.zeros(12)
        st0 = gpsiq.device_eval_stats()
        monkeypatch.setenv("GPSIQ_EVAL", "device" if n >= 48 else "host")
        out = c.generate_batch(continued(b0, carr)[:n], nsamp, fs, ss, carr_out=co)
        monkeypatch.delenv("GPSIQ_EVAL")
        assert (gpsiq.device_eval_stats()[0] > st0[0]) == (n >= 48), n
        assert np.array_equal(out, whole[b0:b0 + n]), f"batch at {b0}"
        b0, carr = b0 + n, co
    # several contexts on one GPU: ctx[0]'s level for every range, the others keep their own
    fresh(ctxs[0], mode, SEED, sigma, 1000, lv)
    fresh(ctxs[1], mode, 1, 5.0, 0, (77, 3))
    fresh(ctxs[2], mode)
    multi = gpsiq.generate_batch_multi(ctxs, desc, nsamp, fs, ss)
    assert np.array_equal(multi, whole)
    probe = synth_blocks(1, 12, seed=2)
    fresh(ctxs[2], mode)
    off = ctxs[2].generate_batch(probe, nsamp, fs, ss)
    ctxs[1].set_noise(1, 5.0, 0)
    ctxs[1].set_nco_mode(mode)                                  # its level is still (77, 3)
    fresh(ctxs[2], mode, 1, 5.0, 0, (77, 3))
    assert np.array_equal(ctxs[1].generate_batch(probe, nsamp, fs, ss), ctxs[2].generate_batch(probe, nsamp, fs, ss))
    assert not np.array_equal(ctxs[2].generate_batch(probe, nsamp, fs, ss), off)
    if mode == NCO_FIXED:
        q = gpsiq.quantize_blocks(desc, fs, nsamp)[0]
        for r in range(3):
            lo, hi = gpsiq.shard_range(nb, r, 3)
            fresh(c, mode, SEED, sigma, 1000 + lo, lv)
            assert np.array_equal(c.generate_quantized(q[lo:hi], nsamp, ss), whole[lo:hi])
        # explicit launches on the resident set, every variant that has the stage
        fresh(c, mode, SEED, sigma, 1000, lv)
        c.set_descriptors(q)
        stride = 2 * nsamp * ss
        buf = torch.zeros(3 * stride, dtype=torch.uint8, device="cuda")
        v = gpsiq.variants()
        for name in ("auto", "generic", "tile", "seg", "segh"):
            buf.zero_()
            c.launch(5, 3, nsamp, ss, buf.data_ptr(), stride, variant=v[name])
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy().view(np.int8).reshape(3, -1), whole[5:8]), name


@pytest.mark.parametrize("how", ["device", "host"])
def test_reference_patches_carry_the_stage(ctxs, how, monkeypatch):
    """GPSIQ_NCO_REFERENCE at 25 Msps, where every block has patched samples: apply_patches recomputes them with noise and level,
    behind the device-evaluated batch and behind the host-evaluated one"""
    nb, fs, sigma = 48, 25e6, 4970.0
    nsamp = int(round(fs / 10))
    desc = synth_blocks(nb, 16, seed=31)
    patchy(desc, fs, nb)
    patches = gpsiq.reference_blocks(desc, fs, nsamp)[1]
    blocks = sorted(set(int(b) for b in patches["block"]))
    assert len(blocks) >= 4
    monkeypatch.setenv("GPSIQ_EVAL", how)
    fresh(ctxs[0], NCO_REFERENCE)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    combos = [(ss, qmax, gpsiq.level_mult(sigma, qmax / 3.0)) for ss, qmax in ((SC08, 127), (SC16, 2047))]
    got = []
    for ss, qmax, mult in combos:
        fresh(ctxs[1], NCO_REFERENCE, SEED, sigma, 5, (mult, qmax))
        st0 = gpsiq.device_eval_stats()
        got.append(ctxs[1].generate_batch(desc, nsamp, fs, ss))
        assert (gpsiq.device_eval_stats()[0] > st0[0]) == (how == "device")
    for b0 in range(0, nb, 8):                                      # all 48 blocks, the noise eight blocks at a time
        z = nr.noise(SEED, sigma, 5 + b0, 8, nsamp)
        for (ss, qmax, mult), g in zip(combos, got):
            want = lr.level(clean[b0:b0 + 8], z, mult, qmax, ss)
            assert np.array_equal(g[b0:b0 + 8], want), (ss, b0)
            for p in patches[(patches["block"] >= b0) & (patches["block"] < b0 + 8)][:16]:      # the patched samples themselves
                b, n = int(p["block"]), int(p["sample"])
                assert np.array_equal(g[b][2 * n:2 * n + 2], want[b - b0][2 * n:2 * n + 2])


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("ss", [SC08, SC16])
def test_level_off_after_on_changes_nothing(ctxs, mode, ss):
    nb, nsamp, fs = 6, 260000, 2.6e6
    desc = synth_blocks(nb, 16, seed=4)
    for seed in (None, 3):
        fresh(ctxs[0], mode, seed, 300.0, 0)
        co0 = np.zeros(16)
        never = ctxs[0].generate_batch(desc, nsamp, fs, ss, carr_out=co0)
        fresh(ctxs[1], mode, seed, 300.0, 0, (30000, 100))
        co1 = np.zeros(16)
        on = ctxs[1].generate_batch(desc, nsamp, fs, ss, carr_out=co1)
        assert not np.array_equal(on, never) and np.array_equal(co0, co1)
        fresh(ctxs[1], mode, seed, 300.0, 0)
        assert np.array_equal(ctxs[1].generate_batch(desc, nsamp, fs, ss), never)


def test_refusals(ctxs):
    import torch
    c = ctxs[0]
    fresh(c, NCO_FIXED)
    for mult, qmax in ((0, 100), (2 ** 24, 100), (65536, 0), (65536, 32768), (65536, -1)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            c.set_level(mult, qmax)
        assert e.value.code == -1, (mult, qmax)
    nsamp = 260000
    desc = synth_blocks(2, 16, seed=8)
    q = gpsiq.quantize_blocks(desc, 2.6e6, nsamp)[0]
    never = c.generate_batch(desc, nsamp, 2.6e6, SC08)            # the refused settings left the level off
    c.set_level(65536, 128)                                        # fits int16, not int8: the rendering call says so
    st = c.noise_state()
    for call in (lambda: c.generate_batch(desc, nsamp, 2.6e6, SC08), lambda: c.generate_block(desc[0], nsamp, 2.6e6, SC08),
                 lambda: c.generate_quantized(q, nsamp, SC08)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            call()
        assert e.value.code == -1
    assert c.noise_state() == st
    c.generate_batch(desc, nsamp, 2.6e6, SC16)
    c.set_level(65536, 127)
    c.set_descriptors(q)
    stride = 4 * nsamp
    buf = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
    v = gpsiq.variants()
    for name in ("rows", "rowsx", "segm", "segb"):
        with pytest.raises(gpsiq.GpsiqError) as e:
            c.launch(0, 2, nsamp, SC16, buf.data_ptr(), stride, variant=v[name])
        assert e.value.code == -5, name
    c.set_level(65536, 128)
    with pytest.raises(gpsiq.GpsiqError) as e:
        c.launch(0, 2, nsamp, SC08, buf.data_ptr(), stride, variant=v["seg"])
    assert e.value.code == -1
    c.level_off()
    assert np.array_equal(c.generate_batch(desc, nsamp, 2.6e6, SC08), never)


def test_runahead_level_flag(tmp_path):
    """gpsiq_runahead --cn0 45 --level 42 at 2.6 Msps int8 writes the stream the restatement predicts from the flag-less int16 file;
    without --level the int8 file is the noise-only stream it has always been."""
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    nblocks, nchan, fs, ns = 4, 8, 2.6e6, 260000
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))

    def run(ss, *flags):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), str(ss), out, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16 if ss == 2 else np.int8).reshape(nblocks, 2 * ns)
    clean16 = run(2)
    sigma = gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs)
    z = nr.noise(7, sigma, 0, nblocks, ns)
    trk_gain = first_block_gains(path, eph, ieph, utc, xyz, sec, nchan)
    mult = lr.level_mult(lr.composite_rms(trk_gain, sigma), 42.0)
    assert np.array_equal(run(1, "--cn0", "45", "--seed", "7", "--level", "42"), lr.level(clean16, z, mult, 127, 1))
    assert np.array_equal(run(1, "--cn0", "45", "--seed", "7", "--level", "42", "--qmax", "7"), lr.level(clean16, z, mult, 7, 1))
    noisy16 = nr.add_noise16(clean16, z)
    assert np.array_equal(run(1, "--cn0", "45", "--seed", "7"), (noisy16 >> 4).astype(np.int8))
    assert np.array_equal(run(2, "--cn0", "45", "--seed", "7"), noisy16)


def first_block_gains(path, eph, ieph, utc, xyz, sec, nchan):
    """gain of every allocated channel in block 0, from the Python pipeline the program is tested against elsewhere"""
    from test_pipeline import WEEK
    from gpsiq.pipeline import RunAheadAllocating
    d = RunAheadAllocating(eph, utc, nchan, WEEK, sec, xyz[0], ieph=ieph).descriptors(xyz[1:])[0]
    return [float(g) for g, p in zip(d["gain"], d["prn"]) if p > 0]
