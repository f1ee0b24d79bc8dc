"""gpsiq_generate_batch_multi at its edges: ranges that are empty or a single block, a timeline that fails in its last range, and
the argument errors -- each against the single-context batch call, and each leaving every context's own settings as they were."""
import numpy as np
import pytest

import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

FS, NS, NC, NDEV = 2.6e6, 2600, 5, 3
E_ARG, E_RANGE = -1, -2
# (seed, sigma, first block) of each context's own receiver noise in the tests that look at what a call leaves behind
OWN = [(5, 40.0, 1000), (9, 25.0, 7), (13, 12.5, 300)]
LEVEL0 = (30000, 100)              # output level of context 0 only


def timeline(nb, seed=71):
    """5 channel slots: slot 1 unused throughout, slot 3 another satellite from the middle of the timeline on"""
    d = synth_blocks(nb, NC, seed=seed)
    d["prn"][:, 1] = 0
    d["prn"][(nb + 1) // 2:, 3] = 27
    d["carr_phase"][(nb + 1) // 2:, 3] = 0.4375
    return d


def float_run(oracle, d, ss):
    """the reference's double-accumulator loop over consecutive blocks, through the oracle's restatement of it"""
    out, carr, prev = [], None, None
    for b in range(len(d)):
        db = d[b].copy()
        if b:
            keep = (prev == db["prn"]) & (db["prn"] > 0)
            db["carr_phase"] = np.where(keep, carr, db["carr_phase"])
        o, carr = oracle.block_float(db, NS, FS, ss)
        out.append(o)
        prev = db["prn"].copy()
    return np.stack(out), carr


@pytest.fixture()
def ctxs():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    cs = [gpsiq.Context(0) for _ in range(NDEV)]
    yield cs
    for c in cs:
        c.close()


def single(mode, d, ss, noise=None, level=None):
    """Context.generate_batch on a fresh context in the same mode -> (samples, carrier phases handed out)"""
    one = gpsiq.Context(0)
    try:
        one.set_nco_mode(mode)
        if noise:
            one.set_noise(*noise)
        if level:
            one.set_level(*level)
        carr = np.zeros(NC)
        return one.generate_batch(d, NS, FS, ss, carr_out=carr), carr
    finally:
        one.close()


def device_ranges(cs, d, ss, ptr_of_empty=0):
    """the call with one device buffer per context (an empty range: pointer 0) -> the ranges' blocks put together"""
    import torch
    nb = len(d)
    ranges = [gpsiq.shard_range(nb, i, len(cs)) for i in range(len(cs))]
    bufs = [torch.zeros((b1 - b0) * 2 * NS * ss, dtype=torch.uint8, device="cuda") if b1 > b0 else None for b0, b1 in ranges]
    gpsiq.generate_batch_multi(cs, d, NS, FS, ss, device_ptrs=[ptr_of_empty if b is None else b.data_ptr() for b in bufs])
    torch.cuda.synchronize()
    parts = [b.cpu().numpy().view(np.int8 if ss == SC08 else np.int16).reshape(-1, 2 * NS) for b in bufs if b is not None]
    return np.concatenate(parts)


@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("nb", [1, 2, 4, 7])
def test_empty_and_single_block_ranges(ctxs, oracle, monkeypatch, nb, mode, ss):
    """1 and 2 blocks over three contexts leave ranges empty, 4 and 7 make ranges of one to three blocks, each several pieces with
    one block per piece: host destination and per-context device destinations == the single-context batch (== the float loop in
    GPSIQ_NCO_REFERENCE), and the same carrier phases handed out."""
    monkeypatch.setenv("GPSIQ_PIECE_BLOCKS", "1")
    d = timeline(nb)
    assert any(b0 == b1 for b0, b1 in (gpsiq.shard_range(nb, i, NDEV) for i in range(NDEV))) == (nb < NDEV)
    want, carr_want = single(mode, d, ss)
    act = d[-1]["prn"] > 0
    ctxs[0].set_nco_mode(mode)
    carr = np.zeros(NC)
    got = gpsiq.generate_batch_multi(ctxs, d, NS, FS, ss, carr_out=carr)
    assert np.array_equal(got, want)
    assert np.array_equal(carr[act], carr_want[act])
    if mode == NCO_REFERENCE:
        ref, carr_ref = float_run(oracle, d, ss)
        assert np.array_equal(got, ref)
        assert np.array_equal(carr[act], carr_ref[act])
    ctxs[0].set_nco_mode(NCO_REFERENCE)              # (forget the carried phases: the same call once more)
    ctxs[0].set_nco_mode(mode)
    assert np.array_equal(device_ranges(ctxs, d, ss), want)


def own_settings(cs):
    for c, o in zip(cs, OWN):
        c.set_noise(*o)
    cs[0].set_level(*LEVEL0)


# code and text of the failing call below, as the library reported them before the multi-context call was reworked
FAILS = {NCO_FIXED: (E_RANGE, "block 6: prn 3: f_code/fs = 0 outside (0, 2) chips/sample"),
         NCO_REFERENCE: (E_RANGE, "block 6: prn 3: f_code/fs = 0 outside (0, 2) chips/sample")}


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_a_failing_range_leaves_nothing_behind(ctxs, monkeypatch, mode):
    """A descriptor outside the NCO format in the last block of the last range: the call fails with the code and text it always
    had, every context keeps its own noise settings and counter, and the same contexts then render the good timeline like a
    single context -- no worker, queue or borrowed setting outlives the failure."""
    monkeypatch.setenv("GPSIQ_PIECE_BLOCKS", "1")
    nb = 7
    d = timeline(nb)
    bad = d.copy()
    assert gpsiq.shard_range(nb, NDEV - 1, NDEV)[1] == nb and bad["prn"][nb - 1, 2] > 0
    bad["f_code"][nb - 1, 2] = 0.0
    ctxs[0].set_nco_mode(mode)
    own_settings(ctxs)
    before = [c.noise_state() for c in ctxs]
    assert before == [tuple(o) for o in OWN]
    with pytest.raises(gpsiq.GpsiqError) as ei:
        gpsiq.generate_batch_multi(ctxs, bad, NS, FS, SC08)
    code, text = FAILS[mode]
    assert ei.value.code == code
    assert str(ei.value) == f"gpsiq error {code}: {text}"
    assert [c.noise_state() for c in ctxs] == before
    want, carr_want = single(mode, d, SC08, noise=OWN[0], level=LEVEL0)
    carr = np.zeros(NC)
    got = gpsiq.generate_batch_multi(ctxs, d, NS, FS, SC08, carr_out=carr)
    assert np.array_equal(got, want)
    act = d[-1]["prn"] > 0
    assert np.array_equal(carr[act], carr_want[act])
    assert [c.noise_state() for c in ctxs] == [(OWN[0][0], OWN[0][1], OWN[0][2] + nb)] + before[1:]


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_argument_errors_leave_the_settings_alone(ctxs, mode):
    """a null device pointer for a range that has blocks, a context listed twice, no destination at all: GPSIQ_E_ARG, and every
    context's noise state is what it was"""
    import ctypes as C
    import torch
    nb = 4
    d = timeline(nb)
    ctxs[0].set_nco_mode(mode)
    own_settings(ctxs)
    before = [c.noise_state() for c in ctxs]
    buf = torch.zeros(2 * 2 * NS, dtype=torch.uint8, device="cuda")

    def no_destination():
        handles = (C.c_void_p * NDEV)(*[c._h for c in ctxs])
        dd = np.ascontiguousarray(d)
        gpsiq._check(gpsiq._generate_batch_multi(handles, NDEV, dd.ctypes.data_as(C.c_void_p), nb, NC, NS, FS, SC08, None, None, None))
    calls = {"null device pointer": lambda: gpsiq.generate_batch_multi(ctxs, d, NS, FS, SC08, device_ptrs=[buf.data_ptr(), buf.data_ptr(), 0]),
             "listed twice": lambda: gpsiq.generate_batch_multi([ctxs[0], ctxs[1], ctxs[0]], d, NS, FS, SC08),
             "no destination": no_destination}
    for name, call in calls.items():
        with pytest.raises(gpsiq.GpsiqError) as ei:
            call()
        assert ei.value.code == E_ARG, (name, str(ei.value))
        assert [c.noise_state() for c in ctxs] == before, name
    torch.cuda.synchronize()
