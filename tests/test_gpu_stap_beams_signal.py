"""What gpsiq_stap_beams is for, on the MI355X: tests/_stap_beams_ref.py's scene -- four elements on a half-wavelength square, four
satellites under the noise, independent receiver noise per element, one broadband jammer stream that gpsiq_mix adds to every element
directly and again D samples later from another direction -- through render, gpsiq_mix, gpsiq_stap_cov, gpsiq_stap_beam_weights,
gpsiq_stap_beams and gpsiq_despread, with the device held to the restatements' bytes at every step (the oracle and
tests/_noise_ref.py for the render, tests/_mix_ref.py, tests/_stap_ref.py, tests/_stap_beams_ref.py, tests/_despread_ref.py), and every
satellite's despread prompt behind its own beam held to keep times its prompt in the clean element, keep the bound
tests/test_stap_beams_ref.py derives and asserts to be above one half.  The four beams come from ONE call.  Two blocks of
tests/_despread_ref.py's 2.6 Msps closed loop.  Run with -m gpu."""
import numpy as np
import pytest

import _stap_beams_ref as br
import gpsiq
from gpsiq.abi import SC16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def device_elements(ctx, sc):
    """render, noise and the jammer's two arrivals on the device, every element held to the restatement's bytes -> the device tensors"""
    import torch
    jam = torch.from_numpy(sc["jam"].view(np.uint8).ravel().copy()).cuda()
    nb, ns, n = br.NB, sc["ns"], sc["n"]
    bufs = []
    try:
        for e in range(br.NELEM):
            buf = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
            ctx.set_noise(sc["seed"] + e, sc["sigma"], 0)
            ctx.set_descriptors(sc["q"][e])
            ctx.launch(0, nb, ns, SC16, buf.data_ptr(), 4 * ns)
            ctx.synchronize()
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), sc["noisy"][e]), ("render", e)
            t = sc["terms"][e]
            ctx.mix(n, 0, [t[0].mixterm(buf.data_ptr()), t[1].mixterm(jam.data_ptr()), t[2].mixterm(jam.data_ptr())], br.MIX_SHIFT, 32767, SC16, buf.data_ptr())
            assert np.array_equal(buf.cpu().numpy().view(np.int16).reshape(-1, 2), sc["jammed"][e]), ("mix", e)
            bufs.append(buf)
    finally:
        ctx.noise_off()
    return bufs


def beams_of(ctx, ptrs, n, w, want):
    """the four beams from ONE call, held to the restatement's bytes and counts -> the device tensors"""
    import torch
    ys = [torch.zeros(4 * n, dtype=torch.uint8, device="cuda") for _ in range(len(w))]
    counts, _ = ctx.stap_beams(ptrs, n, SC16, w, br.SHIFT, SC16, [y.data_ptr() for y in ys])
    for b, y in enumerate(ys):
        assert np.array_equal(y.cpu().numpy().view(np.int16).reshape(-1, 2), want[0][b]), b
    assert np.array_equal(counts, want[1])
    return ys


@pytest.mark.parametrize("kernel", [None, "generic", "mfma"], ids=["default", "generic", "mfma"])
def test_the_chain_on_the_device_is_the_restatements_and_every_beam_keeps_its_satellite(ctx, monkeypatch, kernel):
    import torch
    if kernel is None:
        monkeypatch.delenv("GPSIQ_STAP_BEAMS_KERNEL", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_STAP_BEAMS_KERNEL", kernel)
    sc = br.scene()
    nb, ns, n, seg, nsat = br.NB, sc["ns"], sc["n"], sc["seg"], len(br.PRNS)
    bufs = device_elements(ctx, sc)
    ptrs = [b.data_ptr() for b in bufs]
    cov, _ = ctx.stap_cov(ptrs, n, SC16, br.NTAPS)
    assert np.array_equal(cov, sc["cov"])
    w = gpsiq.stap_beam_weights(cov, n, br.NELEM, br.NTAPS, sc["steers"], ref_tap=0, shift=br.SHIFT)
    assert np.array_equal(w, sc["w"])
    beams_of(ctx, ptrs, n, w, sc["beams_jammed"])                      # the receiver's own call: the jammed elements
    if kernel is not None:
        assert ctx.stap_beams_last_plan()[0] == kernel
    assert ctx.stap_beams_last_plan()[3:6] == (br.NELEM, br.NTAPS, nsat)
    # the same weights on the CLEAN elements: what each beam leaves of each satellite
    clean = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).ravel().copy()).cuda() for x in sc["clean"]]
    ys = beams_of(ctx, [t.data_ptr() for t in clean], n, w, sc["beams_clean"])
    ctx.set_descriptors(sc["q"][0])                                    # the correlator's replicas: element 0's timeline, one slot per satellite

    def prompts(t):
        sums = ctx.despread(0, nb, ns, SC16, t.data_ptr(), 4 * ns, seg)[0]
        return np.array([sums[:, k].ravel()["i"].astype(np.int64).mean() for k in range(nsat)])

    m0 = prompts(clean[0])
    assert np.array_equal(m0, sc["prompt_clean"])
    behind = np.stack([prompts(y) for y in ys])
    assert np.array_equal(behind, sc["prompt_beams"])
    print("own beam over clean", np.round(np.diag(behind) / m0, 3).tolist(), "to keep", np.round(sc["keep"], 3).tolist(),
          "; behind the beam at satellite 0", np.round(behind[0] / m0, 3).tolist())
    for b in range(nsat):
        assert sc["keep"][b] > 0.5 and m0[b] > 0 and behind[b, b] >= sc["keep"][b] * m0[b], b
