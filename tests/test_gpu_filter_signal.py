"""What the filter stage is for, on the MI355X: four satellites rendered noiseless in int16 at 10.4 Msps, low-passed at 1.2 MHz with 65
taps and decimated by 4, searched blind by gpsiq_acquire with the search of tests/test_gpu_acquire.py -- against the same search on a
direct 2.6 Msps rendering of the same descriptors.  The filter's group delay is 32 input samples, exactly 8 output samples.
Run with -m gpu."""
import numpy as np
import pytest

import _acquire_ref as ar
import gpsiq
from gpsiq.abi import SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

NSAMP = 16384                     # samples of the block at 2.6 Msps: four dwells a hop apart and every shift of a millisecond fit
DELAY = 8                         # (65 - 1) / 2 input samples / 4


def test_filtered_and_decimated_stream_acquires_like_a_direct_rendering():
    import torch
    S = ar.SEARCH
    assert 3 * S["hop"] + S["ncoh"] + S["nshift"] <= NSAMP - DELAY
    d = synth_blocks(1, 4, seed=2600, doppler_hz=4400.0, prn0=5)
    prns = [int(p) for p in d["prn"][0]]
    taps = gpsiq.filter_design(10.4e6, 1.2e6, 65, 14)
    steps = gpsiq.acquire_steps(2.6e6, S["f0"], S["df"])
    ctx = gpsiq.Context(0)
    try:
        direct = torch.from_numpy(ctx.generate_batch(d, NSAMP, 2.6e6, SC16).view(np.uint8).ravel()).cuda()
        wide = torch.from_numpy(ctx.generate_batch(d, 4 * NSAMP, 10.4e6, SC16).view(np.uint8).ravel()).cuda()
        narrow = torch.zeros(4 * NSAMP, dtype=torch.uint8, device="cuda")
        nout, clipped, _ = ctx.filter(4 * NSAMP, SC16, wide.data_ptr(), taps, 14, 4, 0, SC16, narrow.data_ptr())
        assert nout == NSAMP and clipped == 0
        cells = {}
        for name, buf in (("direct", direct), ("filtered", narrow)):
            _, power, _, _ = ctx.acquire(NSAMP, SC16, buf.data_ptr(), prns, *steps, S["ndopp"], S["nshift"], S["ncoh"], S["nnoncoh"], S["hop"])
            cells[name] = [gpsiq.acquire_decide(power[p], S["guard"]) for p in range(len(prns))]
            print(name + ": " + ", ".join(f"PRN {prn} bin {c[0]} shift {c[1]} ratio {c[2]:.3f}" for prn, c in zip(prns, cells[name])))
        for prn, a, b in zip(prns, cells["direct"], cells["filtered"]):
            assert a[0] == b[0], (prn, a, b)                                             # the same Doppler bin
            # the direct rendering's shift + 8, within its own nearest-sample chip edge, modulo the code period in samples
            off = (b[1] - a[1] - DELAY) % S["nshift"]
            assert min(off, S["nshift"] - off) <= 1, (prn, a, b)
    finally:
        ctx.close()
