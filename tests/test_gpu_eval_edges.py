"""The device-evaluated batch call (csrc/gpsiq_evaldev.cpp; pack_raw, chain_link_scan, quantize_est, eval_blocks, quantize_fixed,
carry_prefix, compact_blocks, gather_slot, scatter_starts of gpsiq_eval_kernels.hip) against an independent reference, with the
events of a timeline -- a slot changes satellite, goes unused, comes back, Doppler through zero -- engineered onto the edges where
those kernels hand a carry on: every 4 blocks (a thread of carry_prefix), 256 (a wave of it, a chunk of chain_link_scan), 1 024 (a
round), every piece end, the first and the last block of a call.  The work is in the block axis: thousands of blocks of 600 to
2 048 samples.  tests/_eval_edges.py builds the timelines and the references (the oracle's fixed-point forms; the reference's loop,
oracle.block_float, with the carrier handed on in Python), tests/test_eval_edges.py checks both on the CPU.  Every element of
every block is compared; no tolerances.  Where a timeline does not have slots enough for all its events it comes in several parts,
and a case renders every part.  Run with -m gpu.

GPSIQ_PIECE_BLOCKS = n on this path (device_piece_ends of csrc/gpsiq_pieces.h, pinned by tests/piece_plans.cpp; restated in
_eval_edges.piece_ends): the first piece has n blocks, each later one eight times the one before while more than one and a half
such pieces are left; n <= 0 or 2 n > nblocks: one piece.  2 600 blocks: "1" -> 1 9 73 585 2600, "3" -> 3 27 219 1755 2600,
"1024" -> 1024 2600 (a piece starts inside a thread's four blocks, and once exactly on a round edge).  203 blocks: "16" -> 16 203
(187 blocks left are not more than 128 + 64), "8" -> 8 72 203.  2 blocks: "1" -> 1 2 (two pieces: 2 n > nblocks does not hold);
1 block: one piece; 9 blocks: "1" -> 1 9."""
import numpy as np
import pytest

import _eval_edges as ee
import _oracle
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16, elem_dtype

pytestmark = pytest.mark.gpu

FS = ee.FS
KINDS = ["pageable", "pinned", "device"]


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


_want = {}


def want_fixed(orc, nc, part, ss):
    """the fixed-point reference of one part of the 2 600-block timeline: computed once, shared, never written to"""
    key = ("fixed", nc, part, ss)
    if key not in _want:
        _want[key] = ee.fixed_reference(orc, ee.fixed_parts(nc)[part][0], FS, ee.NS_FIXED, ss)
        _want[key].setflags(write=False)
    return _want[key]


def want_float(orc, name, d, ns, ss):
    key = ("float", name, ss)
    if key not in _want:
        _want[key] = ee.float_reference(orc, d, FS, ns, ss)
        for a in _want[key]:
            a.setflags(write=False)
    return _want[key]


def render(ctx, d, ns, ss, mode, monkeypatch, kind="pageable", pieces=None, carr=None, seeded=None):
    """one device-evaluated call into a 0x5A-filled buffer with 64 spare bytes behind it -> (elements [nb][2 ns], statistics
    before, after)"""
    import torch
    monkeypatch.setenv("GPSIQ_EVAL", "device")
    if pieces is None:
        monkeypatch.delenv("GPSIQ_PIECE_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("GPSIQ_PIECE_BLOCKS", str(pieces))
    ctx.set_nco_mode(mode)
    nb, nc = d.shape
    nbytes = nb * 2 * ns * ss
    out = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    keep = None
    # the fill runs on torch's stream and the library renders on non-blocking streams of its own: nothing orders the two but this
    torch.cuda.synchronize()
    if kind == "pageable":
        src = d
    else:
        keep = torch.from_numpy(d.view(np.uint8).reshape(-1).copy())
        keep = keep.pin_memory() if kind == "pinned" else keep.cuda()
        src = (keep.data_ptr(), nb, nc)
    torch.cuda.synchronize()                                    # (the descriptors' copy too)
    before = gpsiq.device_eval_stats()
    if seeded is None:
        ctx.generate_batch(src, ns, FS, ss, device_ptr=out.data_ptr(), carr_out=carr)
    else:
        ctx.generate_seeded(d, ns, FS, ss, seeded, device_ptr=out.data_ptr())
    torch.cuda.synchronize()
    after = gpsiq.device_eval_stats()
    del keep
    assert after[0] == before[0] + 1 and after[5] == before[5], "the device path did not take the call (or fell back)"
    host = out.cpu().numpy()
    assert (host[nbytes:] == 0x5A).all(), "bytes behind the last block were written"
    return host[:nbytes].view(elem_dtype(ss)).reshape(nb, 2 * ns), before, after


def same(got, want, d, what=""):
    assert np.array_equal(got, want), f"{what}: {ee.first_difference(got, want, d)}"


# ---- 1. fixed-point model, scan edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("nc", [16, 5])
def test_fixed_point_scan_edges(ctx, orc, monkeypatch, nc, ss, kind):
    """one piece: thread, wave and round edges of carry_prefix, compact_blocks, pack_raw against the host's pack"""
    for part, (d, rec) in enumerate(ee.fixed_parts(nc)):
        got, _, _ = render(ctx, d, ee.NS_FIXED, ss, NCO_FIXED, monkeypatch, kind, pieces=0)
        same(got, want_fixed(orc, nc, part, ss), d, f"part {part}")


# ---- 2. fixed-point model, piece edges -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pieces", ["1", "3", "1024"])
@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("nc", [16, 5])
def test_fixed_point_piece_edges(ctx, orc, monkeypatch, nc, ss, pieces, kind):
    """the same timeline (a satellite change and an unused run sit on every piece end: test_eval_edges.py) cut into pieces: the
    carry of carry_prefix from piece to piece"""
    assert ee.piece_ends(ee.NB_FIXED, int(pieces)) == {"1": [1, 9, 73, 585, 2600], "3": [3, 27, 219, 1755, 2600], "1024": [1024, 2600]}[pieces]
    for part, (d, rec) in enumerate(ee.fixed_parts(nc)):
        got, _, _ = render(ctx, d, ee.NS_FIXED, ss, NCO_FIXED, monkeypatch, kind, pieces=pieces)
        same(got, want_fixed(orc, nc, part, ss), d, f"part {part}")


# ---- 3. fixed-point model, continuation with mixed cont0 -----------------------------------------------------------------------
@pytest.mark.parametrize("split", [1024, 1023])
@pytest.mark.parametrize("nc", [16, 5])
def test_fixed_point_continuation_with_mixed_slots(ctx, orc, monkeypatch, nc, split):
    """Two calls.  The caller hands the phase of a slot back where the slot goes on with its satellite (what the reference's host
    code does: gps.c keeps carr_phase in the channel, a newly allocated channel gets a new one); a slot that changes satellite at
    the split, one that ends the first call unused and one that starts the second call unused take nothing over.  The
    concatenation is the whole timeline's reference."""
    ss = SC16
    seen = set()
    for part, (d, rec) in enumerate(ee.fixed_parts(nc)):
        a, b = d["prn"][split - 1], d["prn"][split]
        goes_on = (a > 0) & (a == b)
        if part == 0:       # one second call with mixed cont0 (the later parts hold what found no slot in this one)
            assert goes_on.any() and ((b > 0) & ~goes_on).any(), "the second call's cont0 is not mixed"
            assert nc < 16 or (((a == 0) & (b > 0)).any() and ((a > 0) & (b == 0)).any()), "16 slots: all four kinds in one call"
        seen |= {"continues"} if goes_on.any() else set()
        seen |= {"changes"} if ((a > 0) & (b > 0) & (a != b)).any() else set()
        seen |= {"ends unused"} if ((a == 0) & (b > 0)).any() else set()
        seen |= {"starts unused"} if ((a > 0) & (b == 0)).any() else set()
        carr = np.zeros(nc)
        first, _, _ = render(ctx, d[:split], ee.NS_FIXED, ss, NCO_FIXED, monkeypatch, pieces=0, carr=carr)
        d2 = d[split:].copy()
        d2["carr_phase"][0][goes_on] = carr[goes_on]
        second, _, _ = render(ctx, d2, ee.NS_FIXED, ss, NCO_FIXED, monkeypatch, pieces=0)
        same(np.concatenate([first, second]), want_fixed(orc, nc, part, ss), d, f"part {part}")
    assert seen == {"continues", "changes", "ends unused", "starts unused"}, seen


# ---- 4. reference model, link-scan edges ---------------------------------------------------------------------------------------
def reference_case(ctx, orc, monkeypatch, name, parts, ns, ss, kind, pieces, verify=False):
    repaired = expected = 0
    if verify:
        monkeypatch.setenv("GPSIQ_CHAIN_VERIFY", "1")
    else:
        monkeypatch.delenv("GPSIQ_CHAIN_VERIFY", raising=False)
    for part, (d, rec) in enumerate(parts):
        want, _, end = want_float(orc, (name, part), d, ns, ss)
        carr = np.zeros(d.shape[1])
        got, before, after = render(ctx, d, ns, ss, NCO_REFERENCE, monkeypatch, kind, pieces=pieces, carr=carr)
        same(got, want, d, f"part {part}")
        assert carr.tobytes() == end.tobytes(), f"part {part}: carr_out {carr} want {end}"
        # a slot with an active block whose certified map is refused (the host's maps: tests/test_chain_parallel.py holds the
        # device's to them) is the host walker's.  The through-zero slots are such slots (tests/test_eval_edges.py); the exact-tie
        # slot is one from some start states only: a block of 2 048 samples has few binades to tie in
        refused = refused_slots((name, part), d, ns)
        zero = [e["slot"] for e in rec["placed"] if e["key"][0] == "doppler_zero"]
        assert set(zero) <= set(refused)
        assert after[3] - before[3] >= len(refused), f"part {part}: slots {refused} have refused maps, {after[3] - before[3]} slots were repaired"
        expected += len(zero)
        repaired += after[3] - before[3]
    return repaired, expected


def refused_slots(key, d, ns):
    key = ("refused", key)
    if key not in _want:
        ok = gpsiq.chain_maps(gpsiq.chain_inputs(d), FS, ns)[0]["ok"]
        _want[key] = [int(i) for i in np.flatnonzero(((ok == 0) & (d["prn"] > 0)).any(axis=0))]
    return _want[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pieces", [None, "1"])
@pytest.mark.parametrize("ss", [SC08, SC16])
@pytest.mark.parametrize("nc", [16, 1])
def test_reference_link_scan_edges(ctx, orc, monkeypatch, nc, ss, pieces, kind):
    """1 100 blocks, events on the chunk edges of chain_link_scan (256, 512, 768, 1 024), Doppler through zero in the first and in
    the last block of a chunk, a slot unused for a whole chunk: bytes and carr_out are float_reference's.
    chain_link_scan, gather_slot and scatter_starts run ONCE over the whole timeline whatever the piece plan is (phase B of
    gpsiq_evaldev.cpp: b0 = 0, the carry[] of the link scan from launch to launch is never read today); GPSIQ_PIECE_BLOCKS varies
    chain_prepare, quantize_est and the synthesis pieces in front of it.  With the plan unset the head piece follows the measured
    kernel rate (device_piece_ends), so those cases' piece edges are not the same from run to run; "1" pins them.
    NOT observed here: the known / unknown tracking of chain_link_scan from chunk to chunk.  A slot with a block that does not
    link is walked whole by the host, which rewrites every start state of it; only the linked-block count of gpsiq.chain_stats()
    would show it."""
    if pieces is not None:
        assert ee.piece_ends(ee.NB_REFERENCE, int(pieces)) == [1, 9, 73, 585, 1100]
    repaired, expected = reference_case(ctx, orc, monkeypatch, ("edges", nc), ee.reference_parts(nc), ee.NS_REFERENCE, ss, kind, pieces)
    assert expected > 0 and repaired > 0


def test_reference_link_scan_edges_verified(ctx, orc, monkeypatch):
    """GPSIQ_CHAIN_VERIFY=1: every linked block is walked serially too at run time, and the call passes"""
    reference_case(ctx, orc, monkeypatch, ("edges", 16), ee.reference_parts(16), ee.NS_REFERENCE, SC16, "pageable", None, verify=True)


# ---- 5. reference model, short calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", ee.SHORT_BLOCKS)
@pytest.mark.parametrize("nc", [1, 16])
def test_reference_short_calls(ctx, orc, monkeypatch, nc, nb):
    """fewer blocks than a chunk, a workgroup, a piece: 1 and 2 blocks also as GPSIQ_PIECE_BLOCKS = 1 (one piece, and pieces of one
    block), 9 blocks as pieces of 1 and 8"""
    assert ee.piece_ends(1, 1) == [1] and ee.piece_ends(2, 1) == [1, 2] and ee.piece_ends(9, 1) == [1, 9]
    for pieces in [None] + ["1"] * (nb in (1, 2, 9)):
        reference_case(ctx, orc, monkeypatch, ("short", nb, nc), ee.short_parts(nb, nc), ee.NS_SHORT, SC16 if nb % 2 else SC08, "pageable", pieces)


# ---- 6. seeded render at the edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(255, 513), (1023, 1100)])
def test_seeded_render_at_the_edges(ctx, orc, monkeypatch, lo, hi):
    """gpsiq_generate_seeded on a slice that starts in the last block of a chunk / of a round, from float_reference's start states:
    the same blocks of the whole timeline"""
    d, rec = ee.reference_parts(16)[0]
    for ss in (SC08, SC16):
        want, starts, _ = want_float(orc, (("edges", 16), 0), d, ee.NS_REFERENCE, ss)
        got, _, _ = render(ctx, d[lo:hi].copy(), ee.NS_REFERENCE, ss, NCO_REFERENCE, monkeypatch, seeded=starts[lo:hi].copy())
        same(got, want[lo:hi], d[lo:hi], f"blocks {lo}..{hi}")


# ---- 7. launch class from the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pinned", "device"])
@pytest.mark.parametrize("pieces", ee.CLASS_PIECES)
@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
def test_launch_class_reduced_on_the_device(ctx, orc, monkeypatch, mode, pieces, kind):
    """The class the synthesis launch is planned from (most active slots, largest amplitude sum, largest code step) comes from
    pack_raw's wave reductions: 13 active slots only in the last block of a partly filled workgroup, an int16 sum > 32767 in one
    block, a half-row code step in another, all in the last piece.  Then the resident set, launched again with the class the
    call left, gives the same bytes."""
    import torch
    ss, ns, nb = SC16, ee.NS_CLASS, ee.NB_CLASS
    d, where = ee.class_timeline(nb)
    if mode == NCO_FIXED:
        key = ("class", ss)
        if key not in _want:
            _want[key] = ee.fixed_reference(orc, d, FS, ns, ss)
        want = _want[key]
    else:
        want = want_float(orc, "class", d, ns, ss)[0]
    got, _, _ = render(ctx, d, ns, ss, mode, monkeypatch, kind, pieces=pieces)
    same(got, want, d, f"heavy blocks {where}")
    stride = 2 * ns * ss
    buf = torch.full((nb * stride + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.launch(0, nb, ns, ss, buf.data_ptr(), stride, stream=torch.cuda.current_stream().cuda_stream)     # behind the fill
    torch.cuda.synchronize()
    again = buf.cpu().numpy()
    assert (again[nb * stride:] == 0x5A).all()
    same(again[:nb * stride].view(elem_dtype(ss)).reshape(nb, 2 * ns), want, d, "launch on the resident set")


# ---- 8. patch lists past the first copy ----------------------------------------------------------------------------------------
def test_patch_list_past_the_first_copy(ctx, orc, monkeypatch):
    """more than 1 024 patches (asserted for the host path in test_eval_edges.py): the second copy of the list, apply_patches over
    many workgroups with a partly filled last wave"""
    d = ee.patchy_timeline(ee.NB_PATCHY, 16)
    for ss in (SC08, SC16):
        want = want_float(orc, "patchy", d, ee.NS_PATCHY, ss)[0]
        got, before, after = render(ctx, d, ee.NS_PATCHY, ss, NCO_REFERENCE, monkeypatch)
        assert after[4] - before[4] > 1024, after[4] - before[4]
        same(got, want, d)
