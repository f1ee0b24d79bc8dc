"""gpsiq_follow at the 32 satellites the header allows, and on a used context.  One state per PRN 1..32 with staggered starts, chips,
fractions and carrier steps of both signs, through launches of five epochs: the span stops the satellites at different launches, the
record array stops one and the code step's range two (tests/test_stage_contract_cases.py pins the statuses on the restatement), and
records, counts and states equal tests/_follow_ref.py's byte for byte.  gpsiq_follow's buffers are members of the context that only
grow: a context that followed 32 satellites for 64 epochs and then one for two gives, for the small call, the bytes a fresh context
gives, and the large call again its first result.  Run with -m gpu."""
import numpy as np
import pytest

import _contract_cases as cc
import _follow_plan as fp
import _follow_ref as fr
import _oracle
import gpsiq
from gpsiq.abi import SC08, SC16
from test_gpu_follow import same, to_device

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
def test_thirty_two_satellites(ss, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    monkeypatch.setenv("GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH", str(cc.FOLLOW32_KNOB))
    stream, cfg, states, ref = cc.follow32_reference(ss)
    assert len(states) == 32 and tuple(int(s) for s in ref[2]["status"]) == cc.FOLLOW32_EXPECT[ss]
    nsamp, max_epochs = len(stream) // 2, ref[0].shape[1]
    buf, ptr = to_device(stream, 4, 64)
    ctx = gpsiq.Context(0)
    try:
        first = ctx.follow(nsamp, ss, ptr, cfg, states, max_epochs)
        same(first, ref)
        plan = fp.query(nsamp, ss, 32, max_epochs, cc.FOLLOW32_KNOB, int(max(ref[1])))
        assert ctx.follow_last_plan() == (plan.grid, plan.per_launch, plan.launches, plan.record_bytes) and plan.grid == 32 and plan.launches == 3
        again = ctx.follow(nsamp, ss, ptr, cfg, states, max_epochs)
        assert again[0].tobytes() == first[0].tobytes() and again[2].tobytes() == first[2].tobytes() and list(again[1]) == list(first[1])
    finally:
        ctx.close()


def test_large_then_small_equals_fresh():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    big_stream, cfg, big_states, big_ref = cc.follow32_reference(SC16, 48000, 64)
    small_stream = np.random.default_rng(79).integers(-128, 128, size=2 * 3000).astype(np.int8)
    small_state = fr.make_state(31, sample=5, chip=17, code_step=fp.C15, carr_step=-(1 << 45))
    big, big_ptr = to_device(big_stream, 0, 64)
    small, small_ptr = to_device(small_stream, 4, 4)
    used, fresh = gpsiq.Context(0), gpsiq.Context(0)
    try:
        b = used.follow(48000, SC16, big_ptr, cfg, big_states, 64)
        same(b, big_ref)
        records = used.follow_last_plan()[3]
        assert records == 32 * 64 * 96 and max(b[1]) == 64 and min(b[1]) >= 1
        for _ in range(2):
            got, want = used.follow(3000, SC08, small_ptr, cfg, [small_state], 2), fresh.follow(3000, SC08, small_ptr, cfg, [small_state], 2)
            assert list(got[1]) == [2] and got[2]["status"][0] == fr.FULL and used.follow_last_plan()[3] == 2 * 96 < records
            for g, w in zip(got[:3], want[:3]):
                assert g.tobytes() == w.tobytes()
            same(got, fr.follow(_oracle.load_oracle(), small_stream, cfg, [small_state], 2))
        again = used.follow(48000, SC16, big_ptr, cfg, big_states, 64)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:3], b[:3]))
    finally:
        used.close()
        fresh.close()
