"""gpsiq_acquire's buffers are members of the context that only grow: a context that searched a large shape (large digit planes, power
grid and correlations) and then a small one gives, for the small one, the bytes a fresh context gives -- nothing of the large call is
left in what the small one reads or writes back.  Through both kernels.  Run with -m gpu."""
import numpy as np
import pytest

import gpsiq
from gpsiq.abi import SC08, SC16

pytestmark = pytest.mark.gpu


def search(ctx, dev, nsamp, ss, prns, ndopp, nshift, ncoh, nn, hop):
    steps = gpsiq.acquire_steps(2.6e6, -1000.0, 500.0)
    return ctx.acquire(nsamp, ss, dev.data_ptr(), prns, *steps, ndopp, nshift, ncoh, nn, hop, corr=True)[:3]


@pytest.mark.parametrize("kernel", ["mfma", "generic"])
def test_large_then_small_equals_fresh(kernel, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    monkeypatch.setenv("GPSIQ_ACQUIRE_KERNEL", kernel)
    rng = np.random.default_rng(78)
    big_shape = (3000 + 2 * 700 + 640, SC16, list(range(1, 9)), 9, 3000, 640, 3, 700)
    small_shape = (20 + 130 + 64, SC08, [31], 3, 21, 64, 2, 130)
    big = torch.from_numpy(rng.integers(0, 256, size=4 * big_shape[0], dtype=np.uint8)).cuda()
    small = torch.from_numpy(rng.integers(0, 256, size=2 * small_shape[0] + 2, dtype=np.uint8)).cuda()
    used, fresh = gpsiq.Context(0), gpsiq.Context(0)
    try:
        b = search(used, big, *big_shape)
        planes = used.acquire_last_plan()[1]
        assert b[1].shape == (8, 9, 3000) and b[2].shape == (8, 9, 3, 3000) and b[1].all() and (planes > 1 << 18) == (kernel == "mfma")
        for _ in range(2):
            got, want = search(used, small, *small_shape), search(fresh, small, *small_shape)
            assert got[1].shape == (1, 3, 21) and 0 <= used.acquire_last_plan()[1] < max(planes, 1)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes()
        # and the large shape again, after the small one
        assert all(x.tobytes() == y.tobytes() for x, y in zip(search(used, big, *big_shape), b))
    finally:
        used.close()
        fresh.close()
