"""Stream order of gpsiq_agc on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side stream
while the producer of its input still waits there behind a filler, and the null stream is busy until after it returns -- so an upload of
the state, a memset of the per-window slots, one of the three kernels or a copy-back queued on the wrong stream gives wrong bytes, wrong
counts, wrong multipliers or a wrong state.  The second ordered call starts from another state.  And the one wide case: more than 2^30
samples of int8 into int16, a destination past 2^32 bytes.  Run with -m gpu."""
import numpy as np
import pytest

import _agc_ref as ar
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0x7F


@pytest.mark.parametrize("thresh", [0, 127], ids=["blanker-off", "blanker-on"])
def test_agc_runs_behind_the_producer_on_its_stream(ctx, scratch, side, thresh):
    import torch
    rng = np.random.default_rng(6)
    nsamp = 9001
    x = ar.full_range(rng, nsamp, SC08)
    true = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    buf = torch.full((2 * nsamp,), GUARD, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(2 * nsamp + 64, dtype=torch.uint8, device="cuda")
    c = ar.cfg(window=256, navg=3, target_q8=256 * 100, mult0=50000, blank_thresh=thresh, blank_hold=30, qmax=127)
    cfg = ar.to_lib_cfg(c)
    for start in (ar.FRESH, ar.State(((3000000, 512), (90000, 300)), 55555, 100, 77, 12)):
        want = ar.agc_ref(x, c, start, SC08)
        assert want[1] > 0 and (want[2] > 0 or not thresh and start.hold == 0)
        buf.fill_(GUARD)
        dst.fill_(GUARD)
        wrong_state = ar.to_lib_state(start)
        ctx.agc(nsamp, SC08, buf.data_ptr(), cfg, SC08, dst.data_ptr(), state=wrong_state)      # an ordinary call on the wrong input
        assert not np.array_equal(dst.cpu().numpy()[:2 * nsamp].view(np.int8).reshape(-1, 2), want[0]) and ar.from_lib_state(wrong_state) != want[4]
        dst.fill_(GUARD)
        torch.cuda.synchronize()
        st = ar.to_lib_state(start)
        clipped, blanked, mults, _ = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True),
                                             lambda s: ctx.agc(nsamp, SC08, buf.data_ptr(), cfg, SC08, dst.data_ptr(), state=st, stream=s))
        got = dst.cpu().numpy()
        assert np.array_equal(got[:2 * nsamp].view(np.int8).reshape(-1, 2), want[0]) and (got[2 * nsamp:] == GUARD).all()
        assert (clipped, blanked, mults.tolist()) == want[1:4] and ar.from_lib_state(st) == want[4]


def test_more_than_two_to_the_30_samples_into_more_than_two_to_the_32_bytes(ctx):
    """int8 in, int16 out: the sample index passes 2^30 and the byte offset of an output 2^32.  navg 1 and no hold: the multiplier of a
    window follows from the window before it and the blank flags from the sample alone, so the reference restates windows of the span only
    -- the first, those around byte offsets 2^31 and 2^32 of the destination, and the last -- each from one window earlier.  |x| <= 128
    and mult_max = 100 * 65536 keep |y| <= 12800: the clip count must be 0.  A sample is blanked iff one of its elements is -128, which
    the device counts here with torch"""
    import torch
    W = 65536
    nsamp = (1 << 30) + 3 * W + 1000
    torch.manual_seed(33)
    x = torch.randint(-128, 128, (2 * nsamp,), dtype=torch.int8, device="cuda")
    dst = torch.full((4 * nsamp + 64,), GUARD, dtype=torch.uint8, device="cuda")
    c = ar.cfg(window=W, navg=1, target_q8=256 * 5000, mult0=65536, mult_min=1, mult_max=100 * 65536, blank_thresh=127, blank_hold=0, qmax=32767)
    st = gpsiq.AgcState()
    clipped, blanked, mults, ms = ctx.agc(nsamp, SC08, x.data_ptr(), ar.to_lib_cfg(c), SC16, dst.data_ptr(), state=st)
    nwin, fill = ar.span(nsamp, W)
    assert clipped == 0 and len(mults) == nwin and int(st.fill) == fill and int(st.nring) == 1 and int(st.hold) == 0
    assert blanked == int((x.view(-1, 2) == -128).any(dim=1).sum().item())
    out = dst[:4 * nsamp].view(torch.int16).reshape(-1, 2)
    for w in (1, (1 << 29) // W, (1 << 30) // W, nwin - 1):
        lo, hi = (w - 1) * W, min((w + 1) * W, nsamp)
        want = ar.agc_ref(x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2), c, ar.FRESH, SC16)
        got = out[w * W:hi].cpu().numpy()
        assert mults[w] == want[3][1] and np.array_equal(got, want[0][W:]), (w, np.argwhere(got != want[0][W:])[:4])
        assert np.abs(got).max() > 1000
    last = ar.from_lib_state(st)
    assert (last.psum, last.pcnt) == (want[4].psum, want[4].pcnt)
    assert (dst[4 * nsamp:].cpu().numpy() == GUARD).all()
    del x, dst, out
    torch.cuda.empty_cache()
