"""gpsiq_despread's buffers are members of the context that only grow: a context that despread a large shape and then a small one
gives, for the small one, the bytes a fresh context gives (nothing of the large call is left in what the small one reads or
adds into).  Run with -m gpu."""
import numpy as np
import pytest

import gpsiq
from gpsiq.abi import SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu


def despread(ctx, q, nsamp, ss, seg_len, dev, stride):
    ctx.set_descriptors(q)
    return ctx.despread(0, len(q), nsamp, ss, dev.data_ptr(), stride, seg_len, clip=90)[:3]


def test_large_then_small_equals_fresh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    rng = np.random.default_rng(77)
    big_q = gpsiq.quantize_blocks(synth_blocks(12, 16, seed=1), 2.6e6, 30001)[0]
    small_q = gpsiq.quantize_blocks(synth_blocks(2, 3, seed=2), 2.6e6, 4097)[0]
    big = torch.from_numpy(rng.integers(0, 256, size=12 * 4 * 30001, dtype=np.uint8)).cuda()
    small = torch.from_numpy(rng.integers(0, 256, size=2 * (2 * 4097 + 2), dtype=np.uint8)).cuda()
    used, fresh = gpsiq.Context(0), gpsiq.Context(0)
    try:
        b = despread(used, big_q, 30001, SC16, 64, big, 4 * 30001)
        assert b[0].shape == (12, 16, 469) and b[0].view(np.int64).any() and b[2]["sumsq_i"].all()
        for _ in range(2):
            got = despread(used, small_q, 4097, SC08, 2560, small, 2 * 4097 + 2)
            want = despread(fresh, small_q, 4097, SC08, 2560, small, 2 * 4097 + 2)
            assert got[0].shape == (2, 3, 2)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes()
        # and the large shape again, after the small one
        assert all(x.tobytes() == y.tobytes() for x, y in zip(despread(used, big_q, 30001, SC16, 64, big, 4 * 30001), b))
    finally:
        used.close()
        fresh.close()
