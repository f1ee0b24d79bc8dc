"""gpsiq_follow on the MI355X: records, counts and returned states equal tests/_follow_ref.py's restatement of the contract
(include/gpsiq_rows.h, "Follow") byte for byte.  The call is a pure function of (arguments, stream bytes), so the streams are random
elements with the format's extremes at both ends, or one value throughout; the cases are tests/_follow_plan.py's table, whose claims
tests/test_follow_ref.py holds on the CPU.  Every case asserts what the call took against the planner.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import _follow_plan as fp
import _follow_ref as fr
import _oracle
import gpsiq
from gpsiq.abi import FOLLOW_EPOCH_DTYPE, FOLLOW_STATE_DTYPE

pytestmark = pytest.mark.gpu

GUARD = 0x7F


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


def to_device(stream, base=0, guard=0):
    """elements of one span -> (tensor that owns the memory, device pointer with pointer % 16 == base); `guard` bytes of 0x7f behind,
    and every other byte of the allocation 0x7f as well"""
    import torch
    raw = np.ascontiguousarray(stream).view(np.uint8).ravel()
    buf = torch.full((raw.size + guard + 32,), GUARD, dtype=torch.uint8, device="cuda")
    off = (base - buf.data_ptr()) % 16
    buf[off:off + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return buf, buf.data_ptr() + off


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(case, stream, cfg, states, reference outputs) of a case of the table, computed once"""
    c = [k for k in fp.CASES if k.name == name][0]
    return (c,) + fr.materialise(_oracle.load_oracle(), c, fp.CASES.index(c))


def same(got, ref):
    """records (those that were written, and zeros behind them), counts and states"""
    rec, n, st = got[:3]
    assert rec.dtype == FOLLOW_EPOCH_DTYPE and st.dtype == FOLLOW_STATE_DTYPE and rec.shape == ref[0].shape
    assert list(n) == list(ref[1])
    for p in range(len(n)):
        assert rec[p].tobytes() == ref[0][p].tobytes(), (p, [f for f in FOLLOW_EPOCH_DTYPE.names if not np.array_equal(rec[p][f], ref[0][p][f])])
        assert st[p].tobytes() == ref[2][p].tobytes(), (p, [f for f in FOLLOW_STATE_DTYPE.names if not np.array_equal(st[p][f], ref[2][p][f])])


def took(ctx, c, nsamp, ref, knob=None):
    """what the call took, against the planner"""
    plan = fp.query(nsamp, c.ss, len(c.states), c.max_epochs, knob, int(max(ref[1])))
    got = ctx.follow_last_plan()
    assert got == (plan.grid, plan.per_launch, plan.launches, plan.record_bytes), (got, plan)


@pytest.mark.parametrize("name", [c.name for c in fp.CASES])
def test_case_table(ctx, name):
    c, stream, cfg, states, ref = case_reference(name)
    nsamp = len(stream) // 2
    buf, ptr = to_device(stream, c.base, c.guard)
    assert ptr % 16 == c.base
    first = ctx.follow(nsamp, c.ss, ptr, cfg, states, c.max_epochs)
    same(first, ref)
    assert first[3] >= 0.0
    took(ctx, c, nsamp, ref)
    # the call repeated: the same bytes
    again = ctx.follow(nsamp, c.ss, ptr, cfg, states, c.max_epochs)
    assert again[0].tobytes() == first[0].tobytes() and again[2].tobytes() == first[2].tobytes() and list(again[1]) == list(first[1])


@pytest.mark.parametrize("name,knob", [("mixed-int16", 7), ("mixed-int8", 7), ("full", 7), ("mixed-int16", 40), ("mixed-int16", 1), ("range-code", 2), ("no-room", 3)])
def test_relaunches_give_the_same_bytes(ctx, name, knob):
    """GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH: launches of 7 epochs (40 epochs: five full launches and one of five), of exactly the run's
    length (the stop is seen by one more launch), of one epoch, and with satellites that stop at different launches"""
    c, stream, cfg, states, ref = case_reference(name)
    nsamp = len(stream) // 2
    buf, ptr = to_device(stream, c.base, c.guard)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH", str(knob))
        got = ctx.follow(nsamp, c.ss, ptr, cfg, states, c.max_epochs)
    same(got, ref)
    took(ctx, c, nsamp, ref, knob)
    assert ctx.follow_last_plan()[2] == int(max(ref[1])) // knob + 1


@pytest.mark.parametrize("name,cut", [("mixed-int16", 13), ("mixed-int8", 1), ("carrier", 19)])
def test_a_run_cut_and_continued_from_the_returned_state(ctx, name, cut):
    """`cut` epochs (status 2), then from the returned state: the records of one call, and its final state"""
    c, stream, cfg, states, ref = case_reference(name)
    nsamp = len(stream) // 2
    buf, ptr = to_device(stream, c.base, c.guard)
    a = ctx.follow(nsamp, c.ss, ptr, cfg, states, cut)
    assert list(a[1]) == [cut] * len(states) and all(s == fr.FULL for s in a[2]["status"])
    b = ctx.follow(nsamp, c.ss, ptr, cfg, a[2], c.max_epochs)
    for p in range(len(states)):
        whole = np.concatenate([a[0][p, :cut], b[0][p, :b[1][p]]])
        assert whole.tobytes() == ref[0][p, :ref[1][p]].tobytes(), p
    assert b[2].tobytes() == ref[2].tobytes()


def test_a_stream_in_page_locked_host_memory(ctx):
    """the device reads page-locked host memory in place, as it does for the search"""
    c, stream, cfg, states, ref = case_reference("lengths-int8")
    import ctypes as C
    raw = np.ascontiguousarray(stream).view(np.uint8).ravel()
    host = gpsiq._host_alloc(raw.size + 4 + 4096)
    assert host
    try:
        C.memset(host, GUARD, raw.size + 4 + 4096)
        C.memmove(host + 4, raw.ctypes.data, raw.size)
        same(ctx.follow(len(stream) // 2, c.ss, host + 4, cfg, states, c.max_epochs), ref)
    finally:
        gpsiq._host_free(host)


def test_argument_errors(ctx):
    """GPSIQ_E_ARG for everything the header names, before anything is launched; the plan then reads "no call"."""
    c, stream, cfg, states, ref = case_reference("lengths")
    nsamp = len(stream) // 2
    buf, ptr = to_device(stream)

    def bad(nsamp=nsamp, ss=c.ss, ptr=ptr, cfg=cfg, states=states, max_epochs=4, **fields):
        st = np.array(states, copy=True)
        cf = np.array(cfg, copy=True)
        for f, v in fields.items():
            if f in cf.dtype.names:
                cf[f] = v
            else:
                st[f][-1] = v
        with pytest.raises(gpsiq.GpsiqError) as e:
            ctx.follow(nsamp, ss, ptr, cf, st, max_epochs)
        assert e.value.code == -1, fields
        assert ctx.follow_last_plan()[0] is None

    bad(ss=3)
    bad(nsamp=-1)
    bad(ptr=ptr + 2)
    bad(ptr=0)
    bad(max_epochs=0)
    bad(max_epochs=(1 << 30) // 96 // len(states) + 1)
    bad(states=states[:0])
    bad(states=np.concatenate([states] * 7))                 # 35 satellites
    bad(prn=0)
    bad(prn=33)
    bad(chip=1023)
    bad(code_frac=1 << 56)
    bad(code_step0=(1 << 52) - 1)
    bad(code_step0=1 << 57)
    bad(carr_phase=1 << 59)
    bad(carr_int=1 << 59)
    bad(carr_int=-(1 << 59))
    bad(prev_ip=(1 << 22) + 1)
    bad(prev_qp=-(1 << 22) - 1)
    bad(have_prev=2)
    bad(spacing=0)
    bad(spacing=(1 << 56) + 1)
    bad(pull_epochs=-1)
    bad(reserved=1)
    for g in ("kf", "kp", "ki", "kd"):
        bad(**{g: -1})
        bad(**{g: 1 << 46})
    # and the call still works
    same(ctx.follow(nsamp, c.ss, ptr, cfg, states, c.max_epochs), ref)
