"""Stream order of gpsiq_mix on the MI355X, with the apparatus of tests/test_gpu_stage_streams.py: the stage is called on a side stream
while the producer of its inputs still waits there behind a filler, and the null stream is busy until after it returns -- so a table
upload, the zeroing of the count, a kernel or the count's copy-back queued on the wrong stream gives wrong bytes or a wrong count.
The first ordered call is the context's first mix, so it queues the table itself.  And the wide-offset case: one in-place call over
more than 2^31 bytes of int16, filled on the device and compared on windows at its start, across byte 2^31 and at its end.
Run with -m gpu."""
import numpy as np
import pytest

import _mix_ref as mr
import gpsiq
from gpsiq.abi import MIX_ROTATED, MIX_STREAM, MIX_TONE, SC08, SC16
from test_gpu_stage_streams import ctx, ordered, scratch, side  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 0x7F


@pytest.mark.parametrize("kernel", ["generic", "rows"])
def test_mix_runs_behind_the_producer_on_its_stream(scratch, side, monkeypatch, kernel):
    import torch
    monkeypatch.setenv("GPSIQ_MIX_KERNEL", kernel)
    c = gpsiq.Context(0)                                               # a context of its own: the table has not crossed yet
    try:
        rng = np.random.default_rng(12)
        nsamp = 20011
        x, y = mr.full_range(rng, nsamp, SC08), mr.full_range(rng, nsamp - 3, SC16)
        terms = [mr.Term(MIX_STREAM, 1 << 5, x), mr.Term(MIX_ROTATED, 1, y, skip=3, step=-(7 << 50)), mr.Term(MIX_TONE, 9, step=(3 << 50) + 1, gate=(5, 2, 1))]
        want, wc = mr.mix_ref(nsamp, 77, terms, 5, 100, np.int8)
        true_x = torch.from_numpy(x.view(np.uint8).ravel().copy()).cuda()
        true_y = torch.from_numpy(y.view(np.uint8).ravel().copy()).cuda()
        buf, other = torch.full_like(true_x, GUARD), torch.full_like(true_y, GUARD)
        mts = [terms[0].mixterm(buf.data_ptr()), terms[1].mixterm(other.data_ptr()), terms[2].mixterm()]
        torch.cuda.synchronize()

        def produce(s):
            buf.copy_(true_x, non_blocking=True)
            other.copy_(true_y, non_blocking=True)

        for _ in range(2):                                             # the second time with the table in place: count and kernel alone
            gc, _ = ordered(scratch, side, produce, lambda s: c.mix(nsamp, 77, mts, 5, 100, SC08, buf.data_ptr(), stream=s))
            assert c.mix_last_plan()[0] == kernel
            assert np.array_equal(buf.cpu().numpy().view(np.int8).reshape(-1, 2), want) and gc == wc
            buf.fill_(GUARD)
            other.fill_(GUARD)
            torch.cuda.synchronize()
    finally:
        c.close()


def test_a_span_past_two_to_the_31_bytes_in_place(ctx, monkeypatch):
    """Byte offsets pass 2^31 inside the span.  The restatement sees three windows only: the first samples, those either side of
    byte 2^31, and the last; the count is held to theirs from below and to the clamp's reach from above."""
    import torch
    nsamp, m0, win = (1 << 29) + 5003, (1 << 32) - 1000, 4096
    x = torch.empty(2 * nsamp, dtype=torch.int16, device="cuda")
    tone = dict(step=(41 << 50) + 5, rate=-(1 << 30), sweep=(65, 3), gate=(129, 64, 7))
    starts = (0, (1 << 29) - win // 2, nsamp - win)
    for kernel in ("rows", "generic"):
        monkeypatch.setenv("GPSIQ_MIX_KERNEL", kernel)
        torch.manual_seed(33)
        x.random_(-32768, 32768)
        before = [x[2 * s:2 * (s + win)].cpu().numpy().reshape(-1, 2) for s in starts]
        terms = [gpsiq.MixTerm.stream(x.data_ptr(), SC16, 1 << 4), mr.Term(MIX_TONE, 1 << 10, **tone).mixterm()]
        clipped, _ = ctx.mix(nsamp, m0, terms, 4, 32767, SC16, x.data_ptr())
        assert ctx.mix_last_plan()[0] == kernel
        seen = 0
        for s, b in zip(starts, before):
            want, wc = mr.mix_ref(win, m0 + s, [mr.Term(MIX_STREAM, 1 << 4, b), mr.Term(MIX_TONE, 1 << 10, **tone)], 4, 32767, np.int16)
            assert np.array_equal(x[2 * s:2 * (s + win)].cpu().numpy().reshape(-1, 2), want), (kernel, s)
            seen += wc
        assert seen > 0 and seen <= clipped <= 2 * nsamp
    del x
    torch.cuda.empty_cache()
