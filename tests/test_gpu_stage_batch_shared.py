"""The four staged batch calls -- gpsiq_generate_batch_filtered, _packed, _mixed and _resampled -- work through their pieces with ONE
staging ring of the context (csrc/gpsiq_stage_batch.h), which only grows and holds whatever the call before left in it, of whichever
stage.  One used context makes a filtered batch with 257 taps (the lead region in use), a packed batch with an odd nsamp (the rendered
blocks repacked inside the ring), a mixed batch with a tone (in place), a resampled batch at step 5/4 with interpolation, and the
filtered and the packed call again at a smaller shape; each is, byte for byte, count for count and phase for phase, what a fresh
context gives that makes only that call with the same settings.  7 blocks in pieces of 3: both pairs are taken twice, the last piece
is ragged, and a satellite change falls on a piece edge.  Run with -m gpu."""
import numpy as np
import pytest

import gpsiq
from gpsiq.abi import NCO_FIXED, PK4, SC08
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

FS, NB, NSAMP, NC = 10.4e6, 7, 4096, 4
PIECE = 3
FILTER_TAPS = gpsiq.filter_design(FS, 1.2e6, 257, 14)
STEP = 5 << 30                                                       # 5/4 input samples per output
RESAMPLE_TAPS = gpsiq.resample_design(STEP, 0.8, 7, 16, 14)
POS0 = (3 << 32) + (1 << 31) + 12345                                 # the first output inside block 0, off the grid


def descriptors(seed, nb=NB, nc=NC):
    """a satellite change on a piece edge (block 3 with pieces of 3) and an unused slot (tests/test_gpu_filter_batch.py)"""
    d = synth_blocks(nb, nc, seed=seed)
    if nb > 3:
        d["prn"][3:, 1] = 29
        d["carr_phase"][3:, 1] = 0.3125
    d["prn"][:, 2] = 0
    return d


def settings(c, qmax):
    """noise and level on, the level a quarter of qmax (packed: rms 2 of 7), the noise block counter at 5"""
    sigma = gpsiq.noise_sigma_for_cn0(50.0, 1.0, FS)
    c.set_nco_mode(NCO_FIXED)
    c.set_noise(77, sigma, 5)
    c.set_level(gpsiq.level_mult(gpsiq.composite_rms(np.full(3, 0.6), sigma), 2.0 if qmax == 7 else qmax / 4.0), qmax)


def filtered(c, d, nsamp, carr):
    settings(c, 127)
    out, clipped = c.generate_batch_filtered(d, nsamp, FS, SC08, FILTER_TAPS, 12, 4, SC08, carr_out=carr)       # shift 12: a gain of 4, the clamp fires
    return out, clipped, c.filter_last_plan()


def packed(c, d, nsamp, carr):
    settings(c, 7)
    return c.generate_batch_packed(d, nsamp, FS, PK4, carr_out=carr), 0, c.pack_last_plan()


def mixed(c, d, nsamp, carr):
    settings(c, 127)
    tone = gpsiq.MixTerm.tone(9, (37 << 50) + 3, gate=(1000, 400, 17))
    out, clipped = c.generate_batch_mixed(d, nsamp, FS, SC08, 3 << 6, [tone], 6, 100, m0=(1 << 32) - 3 * nsamp - 11, carr_out=carr)
    return out, clipped, c.mix_last_plan()


def resampled(c, d, nsamp, carr):
    settings(c, 127)
    out, clipped = c.generate_batch_resampled(d, nsamp, FS, SC08, RESAMPLE_TAPS, 7, 12, 1, STEP, POS0, SC08, carr_out=carr)
    return out, clipped, c.resample_last_plan()


def result(call, c, d, nsamp):
    carr = np.full(d.shape[1], -1.0)
    out, clipped, plan = call(c, d, nsamp, carr)
    return np.ascontiguousarray(out).tobytes(), int(clipped), carr.tobytes(), plan, c.noise_state()


def test_one_ring_serves_every_stage_in_turn(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    for stage in ("FILTER", "PACK", "MIX", "RESAMPLE"):
        monkeypatch.setenv("GPSIQ_%s_PIECE_BLOCKS" % stage, str(PIECE))
    big, small = descriptors(811), descriptors(812, nb=3)
    used = gpsiq.Context(0)
    try:
        for call, d, nsamp, pieces in ((filtered, big, NSAMP, 3), (packed, big, NSAMP - 1, 3), (mixed, big, NSAMP, 3), (resampled, big, NSAMP, 3),
                                       (filtered, small, 512, 1), (packed, small, 512, 1)):
            got = result(call, used, d, nsamp)
            fresh = gpsiq.Context(0)
            try:
                want = result(call, fresh, d, nsamp)
            finally:
                fresh.close()
            what = (call.__name__, len(d), nsamp)
            assert got[3][3] == pieces and got[3] == want[3], what                      # the plan, its piece count
            assert len(got[0]) > 0 and any(got[0]), what
            assert got[0] == want[0], what                                             # the bytes
            assert got[1] == want[1] and (call is packed or got[1] > 0), what          # the count (the packed call has none: it refuses a clamp)
            assert got[2] == want[2] and got[4] == want[4], what                       # the phases handed out, the noise state
    finally:
        used.close()
