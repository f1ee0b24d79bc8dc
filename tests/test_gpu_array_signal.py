"""What the array stage is for, on the MI355X: four elements on a half-wavelength square, one satellite, independent receiver noise
per element, and a chirp swept across the whole band from one direction -- render, gpsiq_mix, gpsiq_array_cov, gpsiq_array_weights,
gpsiq_array_combine -- with the device held to the numpy restatements at every step (the oracle and tests/_noise_ref.py for the
render, tests/_mix_ref.py, tests/_array_ref.py), the combined stream's power held to v^H R v, and the satellite's despread prompt
behind a steered solution held to the single clean element's.  Four blocks of tests/_despread_ref.py's 2.6 Msps closed loop.
Run with -m gpu."""
import math

import numpy as np
import pytest

import _array_ref as ar
import _despread_ref as dr
import _mix_ref as mr
import _noise_ref as nr
import _oracle
import gpsiq
from gpsiq.abi import MIX_STREAM, MIX_TONE, SC16

pytestmark = pytest.mark.gpu

L = dr.LOOP
NB, NS, SEG, FS = 4, L["nsamp"], L["seg_len"], L["fs"]
N = NB * NS
NELEM = 4
SAT_DIR = (math.pi / 2, 0.0)        # due east along the ground: phases 0, 1/2, 0, 1/2 -- whole steps of the 512-entry carrier table
JAM_DIR = (0.7, 0.3)
JAM_GAIN, JAM_PERIOD = 60, 1021     # amplitude 60 * 250 = 15 000, the whole sampled band every 1 021 samples
SHIFT = 13


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    """the restatements' side of the whole chain, computed once"""
    orc = _oracle.load_oracle()
    sigma = gpsiq.noise_sigma_for_cn0(L["cn0"], L["gain"], FS)
    desc = dr.loop_descriptors()[:NB]
    sat = gpsiq.array_steer(ar.SQUARE, *SAT_DIR)
    jam = gpsiq.array_steer(ar.SQUARE, *JAM_DIR)
    assert np.allclose(sat, [0.0, 0.5, 0.0, 0.5], atol=1e-12) and np.allclose(jam, ar.steer_ref(ar.SQUARE, *JAM_DIR), atol=1e-12)
    sat = np.array([0.0, 0.5, 0.0, 0.5])
    q, clean, noisy, jammed, tones = [], [], [], [], []
    for e in range(NELEM):
        qe, _ = gpsiq.quantize_blocks(gpsiq.array_element(desc, [sat[e], sat[e]]), FS, NS)
        c = np.stack([orc.block_fixed(qe[b], NS, SC16) for b in range(NB)])
        x = nr.add_noise16(c, nr.noise(L["seed"] + e, sigma, 0, NB, NS))
        tone = mr.Term(MIX_TONE, JAM_GAIN, phase0=int(round(jam[e] * 2 ** 59)), step=-(1 << 58), rate=(1 << 59) // JAM_PERIOD, sweep=(JAM_PERIOD, 0))
        y, _ = mr.mix_ref(N, 0, [mr.Term(MIX_STREAM, 1, x.reshape(-1, 2)), tone], 0, 32767, np.int16)
        q.append(qe); clean.append(c.reshape(-1, 2)); noisy.append(x.reshape(-1, 2)); jammed.append(y); tones.append(tone)
    # a half-cycle advance is 256 entries of the carrier table, whose second half is the negated first: the clean elements are +- element 0
    for e in range(NELEM):
        assert np.array_equal(clean[e], clean[0] if e % 2 == 0 else -clean[0])
    cov = ar.cov_ref(jammed)
    return dict(sigma=sigma, sat=sat, jam=jam, q=q, clean=clean, noisy=noisy, jammed=jammed, tones=tones, cov=cov)


def device_elements(ctx, scene):
    """render, noise and jammer on the device, every element held to the restatement's bytes -> the four device tensors"""
    import torch
    bufs = []
    try:
        for e in range(NELEM):
            buf = torch.empty(4 * N, dtype=torch.uint8, device="cuda")
            ctx.set_noise(L["seed"] + e, scene["sigma"], 0)
            ctx.set_descriptors(scene["q"][e])
            ctx.launch(0, NB, NS, SC16, buf.data_ptr(), 4 * NS)
            ctx.synchronize()
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), scene["noisy"][e]), ("render", e)
            ctx.mix(N, 0, [gpsiq.MixTerm.stream(buf.data_ptr(), SC16, 1), scene["tones"][e].mixterm()], 0, 32767, SC16, buf.data_ptr())
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), scene["jammed"][e]), ("mix", e)
            bufs.append(buf)
    finally:
        ctx.noise_off()
    return bufs


def prompt(ctx, scene, ptr):
    """gpsiq_despread of the satellite's slot against element 0's descriptors -> sums [NB * nseg]"""
    ctx.set_descriptors(scene["q"][0])
    return ctx.despread(0, NB, NS, SC16, ptr, 4 * NS, SEG)[0][:, 0].ravel()


@pytest.mark.parametrize("steered", [False, True], ids=["power inversion", "steered"])
def test_the_chain_on_the_device_is_the_restatements(ctx, scene, steered):
    import torch
    bufs = device_elements(ctx, scene)
    ptrs = [b.data_ptr() for b in bufs]
    cov, _ = ctx.array_cov(ptrs, N, SC16)
    assert np.array_equal(cov, scene["cov"])
    w = gpsiq.array_weights(cov, N, steer=scene["sat"] if steered else None, loading=0.0, shift=SHIFT)
    want, wc = ar.combine_ref(scene["jammed"], w, SHIFT, SC16)
    y = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.array_combine(ptrs, N, SC16, w, SHIFT, SC16, y.data_ptr())
    assert np.array_equal(y.cpu().numpy().view(np.int16).reshape(-1, 2), want) and clipped == wc == 0
    # The power of the combined stream against v^H R v = Q / 4^shift, Q the quadratic form of the integer weights.  Every component of
    # y is within 1/2 of a = acc / 2^shift, so |sum y^2 - sum a^2| <= sum |y - a| (|y| + |a|) <= sum (|a| + 1/4) over the 2 N components,
    # and sum |a| <= sqrt(2 N sum a^2) (Cauchy-Schwarz): the bound is sqrt(2 N Q / 4^shift) + N / 2.
    ry, _ = ctx.array_cov([y.data_ptr()], N, SC16)
    qf, qim = ar.quadratic_form(w, cov)
    power = qf / 4.0 ** SHIFT
    bound = math.sqrt(2.0 * N * power) + N / 2.0
    print(f"{'steered' if steered else 'power inversion'}: weights {w.tolist()}, combined power {int(ry[0, 0, 0])}, v^H R v {power:.1f}, bound {bound:.1f}; "
          f"element 0 alone {int(cov[0, 0, 0])}")
    assert qim == 0 and abs(int(ry[0, 0, 0]) - power) <= bound
    assert int(ry[0, 0, 0]) < int(cov[0, 0, 0])                       # e_0 meets either constraint (c_0 = 1): the minimum is below element 0 alone
    # the receiver's view: the satellite behind the jammer, and behind the array
    cn_j, s_j = gpsiq.cn0_estimate(prompt(ctx, scene, ptrs[0]), SEG, FS)
    cn_y, s_y = gpsiq.cn0_estimate(prompt(ctx, scene, y.data_ptr()), SEG, FS)
    print(f"C/N0 of element 0 jammed {cn_j:.2f} dB-Hz (one sigma {s_j:.2f}), of the combined stream {cn_y:.2f} dB-Hz (one sigma {s_y:.2f})")


def test_a_steered_solution_keeps_the_satellite(ctx, scene):
    """The steered weights, computed from the jammed covariance, applied to the four CLEAN elements (no noise, no jammer): x_e = c_e x_0
    exactly (c_e = +-1, see the fixture), so acc = x_0 sum w_e c_e and y = round(x_0 (1 + eps)) with |eps| <= (NELEM / sqrt 2) / 2^shift,
    the constraint's rounding bound.  A component of y is then within 1/2 + |eps| max|x_0| of x_0's, and a despread sum, linear in the
    stream with replica components of at most 250 each (|r_0| + |r_1| <= 250 sqrt 2), moves by at most
    SEG * 250 sqrt 2 * (1/2 + |eps| max |x_0|): the quantisation bound."""
    import torch
    bufs = device_elements(ctx, scene)
    cov, _ = ctx.array_cov([b.data_ptr() for b in bufs], N, SC16)
    w = gpsiq.array_weights(cov, N, steer=scene["sat"], loading=0.0, shift=SHIFT)
    c = np.exp(2j * np.pi * scene["sat"])
    wc = ((w[:, 0].astype(np.int64) + 1j * w[:, 1].astype(np.int64)) * c).sum()
    eps = (NELEM / math.sqrt(2.0)) / (1 << SHIFT)
    assert abs(wc - (1 << SHIFT)) <= NELEM / math.sqrt(2.0) + 1e-6
    clean = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda() for x in scene["clean"]]
    y = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.array_combine([t.data_ptr() for t in clean], N, SC16, w, SHIFT, SC16, y.data_ptr())
    want, _ = ar.combine_ref(scene["clean"], w, SHIFT, SC16)
    got = y.cpu().numpy().view(np.int16).reshape(-1, 2)
    assert clipped == 0 and np.array_equal(got, want)
    peak = int(np.abs(scene["clean"][0]).max())
    assert np.abs(got.astype(np.int64) - scene["clean"][0]).max() <= 0.5 + eps * peak
    p0, py = prompt(ctx, scene, clean[0].data_ptr()), prompt(ctx, scene, y.data_ptr())
    bound = SEG * 250.0 * math.sqrt(2.0) * (0.5 + eps * peak)
    di = np.abs(py["i"].astype(np.int64) - p0["i"].astype(np.int64)).max()
    dq = np.abs(py["q"].astype(np.int64) - p0["q"].astype(np.int64)).max()
    print(f"prompt of the clean element {int(p0['i'].astype(np.int64).mean())}, largest difference behind the steered weights {di} / {dq}, bound {bound:.0f}")
    assert max(di, dq) <= bound and p0["i"].astype(np.int64).mean() > 20 * bound
