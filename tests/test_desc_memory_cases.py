"""tests/_desc_memory.py held to what its names say, on the CPU, through the host quantiser (gpsiq.quantize_blocks): every timeline
but `refused` quantises, `refused` fails with the host quantiser's words for block 30, and the satellite changes, the unused blocks
and the Doppler's sign change are where the table says -- seen in the quantiser's OUTPUT (a slot that seeds takes the block's own
carr_phase, one that continues does not), not only in the descriptors."""
import numpy as np
import pytest

import _desc_memory as dm
import gpsiq
from gpsiq.abi import CHAN_DTYPE


def seeded_from_own_phase(d, q):
    """[nb][nc]: the quantised carrier phase is the block's own carr_phase in the accumulator's format (floor(x 2^59): csrc/gpsiq_nco.h)"""
    own = np.floor(np.ldexp(d["carr_phase"], 59)).astype(np.uint64)
    return q["carr_phase"] == own


def seeds_by_prn(d):
    prn = np.maximum(d["prn"].astype(np.int64), 0)
    s = prn > 0
    s[1:] &= prn[1:] != prn[:-1]
    return prn, s


@pytest.mark.parametrize("name", [n for n in dm.NAMES if n != "refused"])
def test_every_timeline_quantises_and_seeds_where_its_satellites_change(name):
    d = dm.timeline(name)
    assert d.dtype == CHAN_DTYPE and not d.flags.writeable
    q, _ = gpsiq.quantize_blocks(d, dm.FS, dm.NSAMP)
    prn, seeds = seeds_by_prn(d)
    assert np.array_equal(q["prn"], prn)
    own = seeded_from_own_phase(d, q)
    assert own[seeds].all(), "a block that seeds its slot reads its own carr_phase"
    assert not own[(prn > 0) & ~seeds].any(), "a block that continues must not (the fresh phases make that visible)"


def test_shapes_and_the_threshold():
    assert dm.timeline("edges").shape == (40, 6) and dm.timeline("one").shape == (1, 3)
    assert dm.timeline("short-ref").shape == (47, 16) and dm.timeline("long-ref").shape == (48, 16)
    assert dm.NSAMP % 64 != 0 and dm.NSAMP / dm.FS == 0.005
    assert (2 * dm.NSAMP) % 16 == 0                               # int8 and int16 blocks are rendered where they lie (PieceOut::direct)
    assert dm.NB_EDGES * dm.NC_EDGES < 300                        # below the fixed model's threshold for any number of host threads
    assert 0 < dm.CUT < dm.NB_EDGES


def test_edges_holds_its_events_where_the_names_say():
    d = dm.timeline("edges")
    q, _ = gpsiq.quantize_blocks(d, dm.FS, dm.NSAMP)
    prn, seeds = seeds_by_prn(d)
    # a slot whose PRN changes exactly at block 8, and again at block 16
    s = dm.SLOT_CHANGES
    assert dm.CHANGE_AT == (8, 16)
    assert np.flatnonzero(seeds[:, s]).tolist() == [0, 8, 16]
    assert len({int(prn[0, s]), int(prn[8, s]), int(prn[16, s])}) == 3 and (prn[:, s] > 0).all()
    # a slot unused in blocks 0..2 that then starts
    s = dm.SLOT_LATE
    assert (prn[:3, s] == 0).all() and (prn[3:, s] > 0).all() and np.flatnonzero(seeds[:, s]).tolist() == [3]
    assert (q["prn"][:3, s] == 0).all()
    # a slot unused in the last block only: carr_phase_out comes from that block's carr_phase
    s = dm.SLOT_ENDS_UNUSED
    assert prn[-1, s] == 0 and (prn[:-1, s] > 0).all() and d["carr_phase"][-1, s] != 0.0
    # Doppler through zero: the quantised carrier step changes sign at block 20
    s = dm.SLOT_ZERO
    step = q["carr_step"][:, s]
    assert (step[:dm.ZERO_AT] < 0).all() and step[dm.ZERO_AT] == 0 and (step[dm.ZERO_AT + 1:] > 0).all()
    assert np.flatnonzero(seeds[:, s]).tolist() == [0]
    # the other two slots are plain, and no two slots of a block share a satellite
    for s in (dm.SLOT_REFUSED, 5):
        assert np.flatnonzero(seeds[:, s]).tolist() == [0] and (prn[:, s] > 0).all()
    for b in range(dm.NB_EDGES):
        on = prn[b][prn[b] > 0]
        assert len(set(on.tolist())) == len(on)
    # the cut of the continuation test: slots that continue across it, and none that seeds at it
    assert not seeds[dm.CUT].any() and (prn[dm.CUT] > 0).sum() == dm.NC_EDGES


def test_the_reference_timelines_have_a_change_and_an_unused_end():
    for name in ("short-ref", "long-ref"):
        d = dm.timeline(name)
        prn, seeds = seeds_by_prn(d)
        assert np.flatnonzero(seeds[:, 2]).tolist() == [0, d.shape[0] // 2]
        assert prn[-1, 5] == 0 and (prn[:-1, 5] > 0).all()
    assert dm.timeline("one")["prn"].min() > 0


def test_refused_is_edges_but_for_one_descriptor_and_fails_in_the_quantisers_words():
    d, e = dm.timeline("refused"), dm.timeline("edges")
    diff = np.argwhere(d != e)
    assert diff.tolist() == [[dm.REFUSED_AT, dm.SLOT_REFUSED]] and (dm.REFUSED_AT, dm.SLOT_REFUSED) == (30, 2)
    assert d["f_code"][30, 2] == 0.0
    with pytest.raises(gpsiq.GpsiqError, match="block 30.*f_code") as err:
        gpsiq.quantize_blocks(d, dm.FS, dm.NSAMP)
    assert err.value.code == -2, err.value                         # GPSIQ_E_RANGE
    gpsiq.quantize_blocks(d[:30], dm.FS, dm.NSAMP)                  # nothing before block 30 is refused
