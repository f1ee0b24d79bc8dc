"""What the space-time stage is for, on the MI355X: two elements, one satellite under the noise, independent receiver noise per
element, and ONE broadband jammer stream that gpsiq_mix adds to every element twice -- directly, and again D samples later (skip = D)
at another phase0, the reflection -- then gpsiq_stap_cov, gpsiq_stap_weights, gpsiq_stap_combine, with the device held to the numpy
restatements at every step (the oracle and tests/_noise_ref.py for the render, tests/_mix_ref.py, tests/_stap_ref.py), the combined
stream's power held to v^H R v, the residual behind two elements and four taps held at least 20 dB under the residual behind the two
elements alone (the bar of tests/test_stap_ref.py's scene), and the satellite's despread prompt behind a steered solution held to
the single clean element's.  Two blocks of tests/_despread_ref.py's 2.6 Msps closed loop, 133 120 samples: 8 x 8 complex entries are
estimated from sixteen thousand samples each, which leaves the weights within a fraction of a dB of the ideal ones.
Run with -m gpu."""
import math

import numpy as np
import pytest

import _despread_ref as dr
import _mix_ref as mr
import _noise_ref as nr
import _oracle
import _stap_ref as sr
import gpsiq
from gpsiq.abi import MIX_ROTATED, MIX_STREAM, SC16

pytestmark = pytest.mark.gpu

L = dr.LOOP
NB, NS, SEG, FS = 2, L["nsamp"], L["seg_len"], L["fs"]
N = NB * NS
NELEM, NTAPS, D = 2, 4, 2
GAIN, CN0 = 0.2, 55.0               # the satellite at amplitude 50 under noise of sigma 101 a component
SAT = (0.0, 0.5)                    # the satellite's phase at the elements: whole steps of the 512-entry carrier table
JAM_SIGMA = 4500.0                  # the jammer stream, white, a component
JAM_DIRECT, JAM_ECHO = (0.0, 0.25), (0.0, 0.892)       # phases at the elements of the direct arrival and of the reflection, cycles
MIX_SHIFT, G_STREAM, G_DIRECT, G_ECHO = 10, 1 << 10, 4, 3    # the element itself; 4 * 250 / 1024 = 0.98 of the jammer; 0.73 of it, late
SHIFT = 12


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
    sigma = gpsiq.noise_sigma_for_cn0(CN0, GAIN, FS)
    desc = dr.loop_descriptors()[:NB].copy()
    desc["gain"][:, 0] = GAIN
    rng = np.random.default_rng(0x57A9)
    jam = np.clip(np.rint(rng.normal(0.0, JAM_SIGMA, size=(N, 2))), -32767, 32767).astype(np.int16)
    q, clean, noisy, jammed, terms = [], [], [], [], []
    for e in range(NELEM):
        qe, _ = gpsiq.quantize_blocks(gpsiq.array_element(desc, [SAT[e], SAT[e]]), FS, NS)
        c = np.stack([orc.block_fixed(qe[b], NS, SC16) for b in range(NB)])
        x = nr.add_noise16(c, nr.noise(L["seed"] + e, sigma, 0, NB, NS)).reshape(-1, 2)
        t = [mr.Term(MIX_STREAM, G_STREAM, x), mr.Term(MIX_ROTATED, G_DIRECT, jam, phase0=int(round(JAM_DIRECT[e] * 2 ** 59))),
             mr.Term(MIX_ROTATED, G_ECHO, jam, skip=D, phase0=int(round(JAM_ECHO[e] * 2 ** 59)))]
        y, clipped = mr.mix_ref(N, 0, t, MIX_SHIFT, 32767, np.int16)
        assert clipped == 0
        q.append(qe); clean.append(c.reshape(-1, 2)); noisy.append(x); jammed.append(y); terms.append(t)
    assert np.array_equal(clean[1], -clean[0])                         # half a cycle is 256 entries of the table: its second half negated
    return dict(sigma=sigma, q=q, clean=clean, noisy=noisy, jammed=jammed, terms=terms, jam=jam,
                cov=sr.cov_ref(jammed, None, NTAPS), cov1=sr.cov_ref(jammed, None, 1))


def device_elements(ctx, scene):
    """render, noise and the jammer's two arrivals on the device, every element held to the restatement's bytes -> the device tensors"""
    import torch
    jam = torch.from_numpy(scene["jam"].view(np.uint8).ravel().copy()).cuda()
    bufs = []
    try:
        for e in range(NELEM):
            buf = torch.empty(4 * N, dtype=torch.uint8, device="cuda")
            ctx.set_noise(L["seed"] + e, scene["sigma"], 0)
            ctx.set_descriptors(scene["q"][e])
            ctx.launch(0, NB, NS, SC16, buf.data_ptr(), 4 * NS)
            ctx.synchronize()
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), scene["noisy"][e]), ("render", e)
            t = scene["terms"][e]
            ctx.mix(N, 0, [t[0].mixterm(buf.data_ptr()), t[1].mixterm(jam.data_ptr()), t[2].mixterm(jam.data_ptr())], MIX_SHIFT, 32767, SC16, buf.data_ptr())
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), scene["jammed"][e]), ("mix", e)
            bufs.append(buf)
    finally:
        ctx.noise_off()
    return bufs


def prompt(ctx, scene, ptr):
    """gpsiq_despread of the satellite's slot against element 0's descriptors -> sums [NB * nseg]"""
    ctx.set_descriptors(scene["q"][0])
    return ctx.despread(0, NB, NS, SC16, ptr, 4 * NS, SEG)[0][:, 0].ravel()


def combined(ctx, ptrs, xs, w):
    """the combiner on the device, held to the restatement -> (device tensor of y, its power sum |y|^2 by the device's own gpsiq_array_cov)"""
    import torch
    want, wc = sr.combine_ref(xs, None, w, SHIFT, SC16)
    y = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
    clipped, _ = ctx.stap_combine(ptrs, N, SC16, w, SHIFT, SC16, y.data_ptr())
    assert np.array_equal(y.cpu().numpy().view(np.int16).reshape(-1, 2), want) and clipped == wc == 0
    ry, _ = ctx.array_cov([y.data_ptr()], N, SC16)
    return y, int(ry[0, 0, 0])


def test_the_chain_on_the_device_is_the_restatements_and_the_taps_null_the_echo(ctx, scene):
    bufs = device_elements(ctx, scene)
    ptrs = [b.data_ptr() for b in bufs]
    cov, _ = ctx.stap_cov(ptrs, N, SC16, NTAPS)
    cov1, _ = ctx.stap_cov(ptrs, N, SC16, 1)
    assert np.array_equal(cov, scene["cov"]) and np.array_equal(cov1, scene["cov1"])
    powers = {}
    for name, r, ntaps in (("two elements", cov1, 1), ("two elements, four taps", cov, NTAPS)):
        w = gpsiq.stap_weights(r, N, NELEM, ntaps, shift=SHIFT)
        y, power_y = combined(ctx, ptrs, scene["jammed"], w)
        # The power of the combined stream against v^H R v = Q / 4^shift, Q the quadratic form of the integer weights.  Every component
        # of y is within 1/2 of a = acc / 2^shift, so |sum y^2 - sum a^2| <= sum |y - a| (|y| + |a|) <= sum (|a| + 1/4) over the 2 N
        # components, and sum |a| <= sqrt(2 N sum a^2) (Cauchy-Schwarz): the bound is sqrt(2 N Q / 4^shift) + N / 2.
        qf, qim = sr.quadratic_form(w, r)
        power = qf / 4.0 ** SHIFT
        bound = math.sqrt(2.0 * N * power) + N / 2.0
        print(f"{name}: combined power {power_y}, v^H R v {power:.1f}, bound {bound:.1f}; element 0 alone {int(cov1[0, 0, 0])}; "
              f"noise alone {2 * N * scene['sigma'] ** 2:.0f}")
        assert qim == 0 and abs(power_y - power) <= bound
        assert power_y < int(cov1[0, 0, 0])                           # e_0 meets the constraint: the minimum is below element 0 alone
        powers[name] = power_y
        cn, s = gpsiq.cn0_estimate(prompt(ctx, scene, y.data_ptr()), SEG, FS)
        print(f"  C/N0 of the satellite behind it {cn:.2f} dB-Hz (one sigma {s:.2f})")
    gain_db = 10 * math.log10(powers["two elements"] / powers["two elements, four taps"])
    print(f"the taps leave {gain_db:.1f} dB less than the two elements alone")
    assert gain_db >= 20.0


def test_a_steered_solution_keeps_the_satellite(ctx, scene):
    """The steered weights (constraint on tap 0 towards the satellite), computed from the jammed covariance, applied to the two CLEAN
    elements (no noise, no jammer): the device writes the restatement's bytes.  x_1 = -x_0 exactly, so y is x_0 through the one FIR
    g[t] = sum over e of w[e][t] c_e / 2^shift, whose g[0] is 1 to the constraint's rounding bound K / sqrt 2 / 2^shift.  The taps
    behind it are free -- g[D] has modulus about 1, because the weights that cancel the reflection sit there -- but a replica t
    samples late correlates with the code by its autocorrelation, 1 - t * 1.023e6 / fs of the prompt where that is positive and at
    most 1 / 1023 of it beyond a chip: 0.607, 0.213 and nothing at 2.6 Msps.  So the in-phase prompt keeps at least
    1 - sum over t >= 1 of |g[t]| * rho(t) of its size, less 5 % for the sampled code's departure from the triangle; the scene is
    built so that this is more than half."""
    import torch
    bufs = device_elements(ctx, scene)
    cov, _ = ctx.stap_cov([b.data_ptr() for b in bufs], N, SC16, NTAPS)
    w = gpsiq.stap_weights(cov, N, NELEM, NTAPS, steer=SAT, ref_tap=0, shift=SHIFT)
    c = np.exp(2j * np.pi * np.array(SAT))
    g = ((w[:, :, 0].astype(np.int64) + 1j * w[:, :, 1].astype(np.int64)) * c[:, None]).sum(axis=0) / float(1 << SHIFT)
    assert abs(g[0] - 1.0) <= (NELEM * NTAPS / math.sqrt(2.0) + 1e-6) / (1 << SHIFT)
    clean = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda() for x in scene["clean"]]
    y, _ = combined(ctx, [t.data_ptr() for t in clean], scene["clean"], w)
    p0, py = prompt(ctx, scene, clean[0].data_ptr()), prompt(ctx, scene, y.data_ptr())
    m0, my = p0["i"].astype(np.int64).mean(), py["i"].astype(np.int64).mean()
    rho = [max(1.0 - t * 1.023e6 / FS, 1.0 / 1023.0) for t in range(NTAPS)]
    keep = 0.95 - sum(abs(g[t]) * rho[t] for t in range(1, NTAPS))
    print(f"FIR the satellite sees {np.round(g, 4).tolist()}; prompt of the clean element {m0:.0f}, behind the steered weights {my:.0f}, "
          f"to keep {keep:.3f} of it")
    assert keep > 0.5 and m0 > 0 and my >= keep * m0
