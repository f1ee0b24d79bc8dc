"""The staging of gpsiq_generate_batch_packed and the counter of gpsiq_pack are members of the context that only grow: a context that
packed a large batch and then a small one gives, for the small one, the bytes a fresh context gives (nothing of the large call is
left in what the small one reads, adds into or copies out).  Run with -m gpu."""
import numpy as np
import pytest

import gpsiq
from gpsiq.abi import PK2, PK4, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu


def batch(ctx, desc, nsamp, bits):
    ctx.set_noise(3, gpsiq.noise_sigma_for_cn0(45.0, 1.0, 2.6e6), 0)
    ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], gpsiq.noise_sigma_for_cn0(45.0, 1.0, 2.6e6)), 2.0 if bits == PK4 else 1.0),
                  7 if bits == PK4 else 1)
    carr = np.zeros(desc.shape[1])
    out = ctx.generate_batch_packed(desc, nsamp, 2.6e6, bits, carr_out=carr)
    return out.copy(), carr, ctx.pack_last_plan()


def test_large_then_small_equals_fresh(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    big, small = synth_blocks(24, 16, seed=1), synth_blocks(3, 5, seed=2)
    rng = np.random.default_rng(5)
    stream = torch.from_numpy(rng.integers(0, 256, size=4 * 4 * 30001, dtype=np.uint8)).cuda()
    packed = torch.zeros(4 * 30004, dtype=torch.uint8, device="cuda")
    used, fresh = gpsiq.Context(0), gpsiq.Context(0)
    try:
        monkeypatch.setenv("GPSIQ_PACK_PIECE_BLOCKS", "9")           # three pieces of the large call, both staging pairs in use
        b = batch(used, big, 26000, PK4)
        assert b[0].shape == (24, 26000) and b[0].any() and b[2][3] == 3
        count_big = used.pack(4, 30001, SC16, stream.data_ptr(), 4 * 30001, PK4, packed.data_ptr(), 30004)[0]
        assert count_big > 0
        for _ in range(2):
            for bits in (PK2, PK4):
                got, want = batch(used, small, 2600, bits), batch(fresh, small, 2600, bits)
                assert got[0].shape == (3, gpsiq.packed_block_bytes(2600, bits)) and got[2] == want[2]
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            # the counter: a small all-in-range stream after the large clamped one counts 0 on both
            zero = torch.zeros(64, dtype=torch.uint8, device="cuda")
            assert used.pack(1, 32, 1, zero.data_ptr(), 64, PK2, packed.data_ptr(), 16)[0] == 0
            assert fresh.pack(1, 32, 1, zero.data_ptr(), 64, PK2, packed.data_ptr(), 16)[0] == 0
        # and the large shapes again, after the small ones
        again = batch(used, big, 26000, PK4)
        assert again[0].tobytes() == b[0].tobytes() and again[1].tobytes() == b[1].tobytes()
        assert used.pack(4, 30001, SC16, stream.data_ptr(), 4 * 30001, PK4, packed.data_ptr(), 30004)[0] == count_big
    finally:
        used.close()
        fresh.close()
