"""Receiver noise on the MI355X: the kernels' zI/zQ equal the numpy restatement (tests/_noise_ref.py) bit for bit, alone and over
the signal, in both NCO models and every core (int8 fields, int16 plain-add and packed), however a timeline is split into calls;
its statistics; and noise off leaves everything as it was.  Run with -m gpu."""
import numpy as np
import pytest

import _noise_ref as nr
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

SEED, SIGMA = 0x5EED, 37.5


@pytest.fixture(scope="module")
def ctxs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    cs = [gpsiq.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def fresh(ctx, mode, seed=None, sigma=0.0, next_block=0):
    ctx.set_nco_mode(mode)
    if seed is None:
        ctx.noise_off()
    else:
        ctx.set_noise(seed, sigma, next_block)


def z16(seed, sigma, block0, nblocks, nsamp):
    return nr.noise(seed, sigma, block0, nblocks, nsamp)


def diff16(noisy, clean):
    """(noisy - clean) mod 2^16 as signed values, shaped [nblocks, nsamp, 2]"""
    d = (noisy.astype(np.int64) - clean.astype(np.int64)) % 65536
    d = np.where(d >= 32768, d - 65536, d)
    return d.reshape(noisy.shape[0], -1, 2)


def wrap16(z):
    return np.where(z % 65536 >= 32768, z % 65536 - 65536, z % 65536)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("block0", [0, 10**9])
def test_pure_noise_equals_numpy(ctxs, mode, block0):
    desc = synth_blocks(4, 16, seed=11)
    desc["gain"] = 0.0
    nsamp = 260000
    fresh(ctxs[0], mode, SEED, SIGMA, block0)
    out = ctxs[0].generate_batch(desc, nsamp, 2.6e6, SC16)
    want = wrap16(z16(SEED, SIGMA, block0, 4, nsamp))
    assert np.array_equal(out.astype(np.int64).reshape(4, nsamp, 2), want)
    assert ctxs[0].noise_state() == (SEED, SIGMA, block0 + 4)


def render_device(ctx, desc, nsamp, fs, ss, blocks):
    import torch
    nb = desc.shape[0]
    buf = torch.empty(nb * 2 * nsamp * ss, dtype=torch.uint8, device="cuda")
    ctx.generate_batch(desc, nsamp, fs, ss, device_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    rows = buf.view(nb, 2 * nsamp * ss)
    dt = np.int16 if ss == SC16 else np.int8
    return {b: rows[b].cpu().numpy().view(dt) for b in blocks}


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("fs", [0.8e6, 1.5e6, 2.6e6, 10e6, 25e6])     # generic, segh, seg
def test_noise_over_signal(ctxs, mode, fs):
    nb, nsamp = 48, int(round(fs / 10))
    desc = synth_blocks(nb, 16, seed=int(fs) % 1000 + mode)
    if mode == NCO_REFERENCE:
        # two channels a hair short of a chip edge at a whole number of samples per chip: the reference's double accumulator
        # and the closed form then disagree now and then (10 Msps: 5 patches, 25 Msps: 29), so the patch kernel adds noise too
        rng = np.random.default_rng(int(fs))
        desc["code_phase"][:, :2] = (rng.integers(0, 1023, (nb, 2)) + 1.0 - 1e-10) % 1023.0
        desc["f_code"][:, :2] = fs / 7
    check = [0, 1, nb - 1]
    if mode == NCO_REFERENCE and fs >= 10e6:
        patches = gpsiq.reference_blocks(desc, fs, nsamp)[1]
        assert len(patches) > 0
        check = sorted(set(check) | set(int(b) for b in patches["block"][:4]))       # the patched samples carry the noise too
    fresh(ctxs[0], mode)
    clean = render_device(ctxs[0], desc, nsamp, fs, SC16, check)
    fresh(ctxs[1], mode, SEED, 1600.0, 77)
    st0 = gpsiq.device_eval_stats()
    noisy = render_device(ctxs[1], desc, nsamp, fs, SC16, check)
    st1 = gpsiq.device_eval_stats()
    for b in check:
        got = diff16(noisy[b][None], clean[b][None])[0]
        assert np.array_equal(got, wrap16(z16(SEED, 1600.0, 77 + b, 1, nsamp)[0])), f"block {b}"
    if mode == NCO_REFERENCE and fs >= 10e6:
        assert st1[0] > st0[0] and st1[4] > st0[4], "the reference-model call should have taken the device path with patches"


@pytest.mark.parametrize("nact", [16, 12])
def test_int8_is_the_int16_sum_shifted(ctxs, nact):
    nb, nsamp, fs = 3, 260000, 2.6e6
    desc = synth_blocks(nb, 16, seed=5)
    desc["gain"] = 1.0
    desc["prn"][:, nact:] = 0
    fresh(ctxs[0], NCO_FIXED)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    fresh(ctxs[1], NCO_FIXED, SEED, 900.0, 3)
    got = ctxs[1].generate_batch(desc, nsamp, fs, SC08)
    s16 = wrap16(clean.astype(np.int64).reshape(nb, nsamp, 2) + z16(SEED, 900.0, 3, nb, nsamp))
    want = (s16 >> 4).astype(np.int8).reshape(nb, 2 * nsamp)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("side", [-16, 16])
def test_int16_cores_either_side_of_the_bound(ctxs, side):
    """max_amplitude + max|z| <= 32767 takes the plain-add core, above it the packed one: both exact."""
    nb, nsamp, fs, sigma = 2, 260000, 2.6e6, 1000.0
    max_z = int(nr.tables(sigma)[1][63])
    amp = (32767 - max_z + side) // 16 + (1 if side > 0 else 0)
    desc = synth_blocks(nb, 16, seed=9)
    desc["gain"] = amp / 250.0 + 1e-9
    assert (16 * int(250 * desc["gain"][0, 0]) + max_z <= 32767) == (side < 0)
    fresh(ctxs[0], NCO_FIXED)
    clean = ctxs[0].generate_batch(desc, nsamp, fs, SC16)
    fresh(ctxs[1], NCO_FIXED, 1, sigma, 0)
    got = ctxs[1].generate_batch(desc, nsamp, fs, SC16)
    assert np.array_equal(diff16(got, clean), wrap16(z16(1, sigma, 0, nb, nsamp)))


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_split_invariance(ctxs, mode, monkeypatch):
    nb, nsamp, fs = 64, 260000, 2.6e6
    desc = synth_blocks(nb, 12, seed=21)
    c = ctxs[0]
    fresh(c, mode, SEED, SIGMA, 1000)
    whole = c.generate_batch(desc, nsamp, fs, SC16)
    assert c.noise_state()[2] == 1000 + nb

    def continued(b, carr):
        d = desc[b:].copy()
        if carr is not None:
            d["carr_phase"][0] = carr
        return d

    # block calls
    fresh(c, mode, SEED, SIGMA, 1000)
    carr = None
    for b in range(nb):
        out, carr = c.generate_block(continued(b, carr)[0], nsamp, fs, SC16)
        assert np.array_equal(out, whole[b]), f"block call {b}"
    # batches of mixed sizes, the short ones through the host quantiser / walker, the long one through the device's
    fresh(c, mode, SEED, SIGMA, 1000)
    b0, carr = 0, None
    for n in (1, 5, 50, 8):
        co = np.zeros(12)
        st0 = gpsiq.device_eval_stats()
        monkeypatch.setenv("GPSIQ_EVAL", "device" if n >= 48 else "host")
        out = c.generate_batch(continued(b0, carr)[:n], nsamp, fs, SC16, carr_out=co)
        monkeypatch.delenv("GPSIQ_EVAL")
        assert (gpsiq.device_eval_stats()[0] > st0[0]) == (n >= 48), n
        assert np.array_equal(out, whole[b0:b0 + n]), f"batch at {b0}"
        b0, carr = b0 + n, co
    assert c.noise_state()[2] == 1000 + nb
    # several contexts on one GPU: ctx[0]'s settings and numbering
    fresh(ctxs[0], mode, SEED, SIGMA, 1000)
    fresh(ctxs[1], mode, 1, 5.0, 0)
    fresh(ctxs[2], mode)
    multi = gpsiq.generate_batch_multi(ctxs, desc, nsamp, fs, SC16)
    assert np.array_equal(multi, whole)
    assert ctxs[0].noise_state()[2] == 1000 + nb and ctxs[1].noise_state() == (1, 5.0, 0)
    if mode == NCO_FIXED:
        # quantised shards, each numbered from its first block
        q = gpsiq.quantize_blocks(desc, fs, nsamp)[0]
        for r in range(3):
            lo, hi = gpsiq.shard_range(nb, r, 3)
            fresh(c, mode, SEED, SIGMA, 1000 + lo)
            assert np.array_equal(c.generate_quantized(q[lo:hi], nsamp, SC16), whole[lo:hi])


def test_statistics(ctxs):
    nb, nsamp, sigma = 10, 260000, 1000.0
    desc = synth_blocks(nb, 8, seed=3)
    desc["gain"] = 0.0
    fresh(ctxs[0], NCO_FIXED, 17, sigma, 0)
    z = ctxs[0].generate_batch(desc, nsamp, 2.6e6, SC16).astype(np.float64).reshape(nb, nsamp, 2)
    fresh(ctxs[0], NCO_FIXED, 18, sigma, 0)
    z2 = ctxs[0].generate_batch(desc, nsamp, 2.6e6, SC16).astype(np.float64).reshape(nb, nsamp, 2)
    zi, zq = z[..., 0].ravel() / sigma, z[..., 1].ravel() / sigma
    n = zi.size
    bound = 5.0 / np.sqrt(n)
    assert abs(zi.var() - 1.0) < 0.005 and abs(zq.var() - 1.0) < 0.005
    assert abs(zi.mean()) < bound and abs(zq.mean()) < bound
    for lag in range(1, 131):
        assert abs(np.mean(zi[:-lag] * zi[lag:])) < bound, lag
        assert abs(np.mean(zq[:-lag] * zq[lag:])) < bound, lag
    assert abs(np.mean(zi * zq)) < bound
    a, b = z[:-1, :, 0].ravel() / sigma, z[1:, :, 0].ravel() / sigma
    assert abs(np.mean(a * b)) < 5.0 / np.sqrt(a.size)
    assert abs(np.mean(zi * z2[..., 0].ravel() / sigma)) < bound


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_noise_off_after_on_changes_nothing(ctxs, mode):
    nb, nsamp, fs = 6, 260000, 2.6e6
    desc = synth_blocks(nb, 16, seed=4)
    fresh(ctxs[0], mode)
    co0 = np.zeros(16)
    never = ctxs[0].generate_batch(desc, nsamp, fs, SC08, carr_out=co0)
    fresh(ctxs[1], mode, SEED, 300.0, 0)
    co1 = np.zeros(16)
    noisy = ctxs[1].generate_batch(desc, nsamp, fs, SC08, carr_out=co1)
    assert not np.array_equal(noisy, never)
    assert np.array_equal(co0, co1), "noise must not touch the carrier state"
    ctxs[1].noise_off()
    fresh(ctxs[1], mode)
    assert np.array_equal(ctxs[1].generate_batch(desc, nsamp, fs, SC08), never)


def test_variant_refusal_and_the_counter(ctxs):
    import torch
    c = ctxs[0]
    nsamp = 260000
    desc = synth_blocks(2, 16, seed=8)
    q = gpsiq.quantize_blocks(desc, 2.6e6, nsamp)[0]
    fresh(c, NCO_FIXED, 3, 50.0, 40)
    c.set_descriptors(q)
    stride = 4 * nsamp
    buf = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
    v = gpsiq.variants()
    for name in ("rows", "rowsx", "segm", "segb"):
        with pytest.raises(gpsiq.GpsiqError) as e:
            c.launch(0, 2, nsamp, SC16, buf.data_ptr(), stride, variant=v[name])
        assert e.value.code == -5
    for name in ("auto", "generic", "tile", "seg"):
        buf.zero_()
        c.launch(1, 1, nsamp, SC16, buf.data_ptr(), stride, variant=v[name])
        torch.cuda.synchronize()
        clean_free = buf[:stride].cpu().numpy().view(np.int16)
        fresh(c, NCO_FIXED)
        c.set_descriptors(q)
        buf.zero_()
        c.launch(1, 1, nsamp, SC16, buf.data_ptr(), stride, variant=v[name])
        torch.cuda.synchronize()
        clean = buf[:stride].cpu().numpy().view(np.int16)
        assert np.array_equal(diff16(clean_free[None], clean[None])[0], wrap16(z16(3, 50.0, 41, 1, nsamp)[0])), name
        fresh(c, NCO_FIXED, 3, 50.0, 40)
        c.set_descriptors(q)
    assert c.noise_state()[2] == 40, "an explicit launch leaves the counter alone"
    c.generate_batch(desc, nsamp, 2.6e6, SC16)
    assert c.noise_state()[2] == 42


def test_runahead_cn0_flag(tmp_path):
    """gpsiq_runahead --cn0 45 --seed 7: the file minus the flag-less file is the noise at gpsiq_noise_sigma_for_cn0(45, 1.0, fs)."""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    nblocks, nchan, fs, ns = 4, 8, 2.6e6, 260000
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))

    def run(*flags):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), "2", out, *flags], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16).reshape(nblocks, 2 * ns)
    clean, noisy = run(), run("--cn0", "45", "--seed", "7")
    sigma = gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs)
    assert np.array_equal(diff16(noisy, clean), wrap16(z16(7, sigma, 0, nblocks, ns)))
