"""Stream order of gpsiq_cfilter on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side
stream while the producer of its input still waits there behind a filler, and the null stream is busy until after it returns -- so
a coefficient upload, a memset of the counter, a kernel or a copy-back queued on the wrong stream gives wrong bytes or a wrong count.
The caller overwrites its taps as soon as the call has returned, and a second ordered call uses different taps.  And the one
wide-offset case: 2^30 + 5000 int16 samples in and out, byte offsets past 2^32 on both sides, filled on the device.  Run with -m gpu."""
import numpy as np
import pytest

import _cfilter_ref as cr
from gpsiq.abi import SC08, SC16
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0x7F
NAMES = {("generic", SC08): "generic", ("generic", SC16): "generic", ("mfma", SC08): "mfma", ("mfma", SC16): "mfma16"}


@pytest.mark.parametrize("kernel,in_size", sorted(NAMES))
def test_cfilter_runs_behind_the_producer_on_its_stream(ctx, scratch, side, monkeypatch, kernel, in_size):
    import torch
    monkeypatch.setenv("GPSIQ_CFILTER_KERNEL", kernel)
    rng = np.random.default_rng(5)
    nsamp, decim, phase, shift = 9001, 3, 1, 6 if in_size == SC08 else 14
    x = cr.full_range(rng, nsamp, in_size)
    true = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
    buf = torch.full((2 * nsamp * in_size,), GUARD, dtype=torch.uint8, device="cuda")
    nout = cr.span(nsamp, decim, phase)[0]
    dst = torch.zeros(2 * nout + 64, dtype=torch.uint8, device="cuda")
    for seed in (1, 2):                                                # the second call: different taps
        taps = np.random.default_rng(seed).integers(-250, 251, size=(65, 2)).astype(np.int16)
        want, wc = cr.cfilter_ref(x, None, taps, shift, decim, phase, SC08)
        assert wc > 0
        mine = taps.copy()
        buf.fill_(GUARD)
        dst.fill_(GUARD)
        ctx.cfilter(nsamp, in_size, buf.data_ptr(), mine, shift, decim, phase, SC08, dst.data_ptr())   # an ordinary call on the wrong input
        wrong = dst.cpu().numpy()[:2 * nout].view(np.int8).reshape(-1, 2)
        assert not np.array_equal(wrong, want)
        dst.fill_(GUARD)
        torch.cuda.synchronize()

        def stage(s):
            out = ctx.cfilter(nsamp, in_size, buf.data_ptr(), mine, shift, decim, phase, SC08, dst.data_ptr(), stream=s)
            mine[:] = 0                                                # the caller's taps are the caller's again
            return out

        n, clipped, _ = ordered(scratch, side, lambda s: buf.copy_(true, non_blocking=True), stage)
        got = dst.cpu().numpy()
        assert ctx.cfilter_last_plan()[0] == NAMES[kernel, in_size]
        assert n == nout and clipped == wc and np.array_equal(got[:2 * nout].view(np.int8).reshape(-1, 2), want) and (got[2 * nout:] == GUARD).all()


def test_a_span_whose_byte_offsets_pass_two_to_the_32(ctx, monkeypatch):
    """int16 in and out, decim 1, 2^30 + 5000 samples: sample 2^30 lies at byte 2^32 of the source and of the destination.  Both
    kernels; the reference filters windows only: the first outputs, those either side of the seam, and the last.  Full-range input
    against taps whose sum is 12 at shift 4: nothing is clamped"""
    import torch
    nsamp, shift = (1 << 30) + 5000, 4
    taps = np.array([[5, -2], [-1, 3], [1, 0]], np.int16)
    torch.manual_seed(32)
    x = torch.randint(-32768, 32768, (2 * nsamp,), dtype=torch.int16, device="cuda")
    dst = torch.empty(4 * nsamp + 64, dtype=torch.uint8, device="cuda")
    seam = 1 << 30
    outputs = list(range(0, 40)) + list(range(seam - 20, seam + 20)) + list(range(nsamp - 40, nsamp))
    x_at = lambda lo, hi: x[2 * lo:2 * hi].cpu().numpy().reshape(-1, 2)
    want = cr.cfilter_windows(x_at, nsamp, taps, shift, 1, 0, SC16, outputs)
    idx = torch.tensor(outputs, device="cuda")
    for kernel, name in (("generic", "generic"), ("mfma", "mfma16")):
        monkeypatch.setenv("GPSIQ_CFILTER_KERNEL", kernel)
        dst.fill_(GUARD)
        n, clipped, ms = ctx.cfilter(nsamp, SC16, x.data_ptr(), taps, shift, 1, 0, SC16, dst.data_ptr())
        assert n == nsamp and ctx.cfilter_last_plan()[0] == name
        got = dst[:4 * nsamp].view(torch.int16).reshape(-1, 2)[idx].cpu().numpy()
        assert np.array_equal(got, want), (kernel, np.argwhere(got != want)[:4])
        assert (dst[4 * nsamp:].cpu().numpy() == GUARD).all() and clipped == 0
        assert int((dst[:4 * nsamp].view(torch.int16) == 0x7F7F).sum().item()) < nsamp // 1000      # the span was written, not left as guards
    del x, dst
    torch.cuda.empty_cache()
