"""gpsiq_generate_batch held to what include/gpsiq.h says about where its descriptors may lie -- pageable, page-locked or device
memory of the context's device -- on EVERY path of the call, not only the one the device takes: the library's own decision on both
sides of its thresholds, GPSIQ_EVAL=host (one kernel, and the piece loop of the fixed model), GPSIQ_CHAIN=device / host,
GPSIQ_EVAL=device at the shapes where the first block is the last and the last block has an unused slot, a call continued from
device-resident rows, a refused descriptor, a base that is only 8-byte aligned; and the pointers the calls must refuse (device
memory handed to the calls that read ch on the host, another device's memory).  The timelines: tests/_desc_memory.py.

The reference of every case is the same call with PAGEABLE descriptors under GPSIQ_EVAL=host (held element for element to the
reference program by tests/test_gpu_reference_nco.py and test_gpu_device_eval.py); one case is held to the reference's own loop
directly.  Every byte and every bit of carr_out must be equal: there is no tolerance anywhere.  Which path took a call is read
from gpsiq.device_eval_stats()[0] -- a case that silently went the other way fails."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _desc_memory as dm
import _pack_ref as pr
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16, SINK_IQFILE
from test_gpu_device_eval import render

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, NS = dm.FS, dm.NSAMP
MODES = [NCO_FIXED, NCO_REFERENCE]
KINDS = ["pinned", "device"]
SIZES = [SC08, SC16]
KNOBS = ("GPSIQ_EVAL", "GPSIQ_CHAIN", "GPSIQ_PIECE_BLOCKS", "GPSIQ_TRACE")


@pytest.fixture()
def ctx(monkeypatch):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    for k in KNOBS:                                     # every test sets the ones it is about
        monkeypatch.delenv(k, raising=False)
    c = gpsiq.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case_reference(name, mode, ss):
    """(bytes, carr_out) of the timeline in one call with pageable descriptors under GPSIQ_EVAL=host, on a context of its own;
    computed once per module and read-only"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ["GPSIQ_EVAL"] = "host"
    c = gpsiq.Context(0)
    try:
        c.set_nco_mode(mode)
        d = dm.timeline(name)
        carr = np.zeros(d.shape[1])
        out = c.generate_batch(d, NS, FS, ss, carr_out=carr).view(np.uint8).reshape(-1)
    finally:
        c.close()
        del os.environ["GPSIQ_EVAL"]
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    out.setflags(write=False)
    carr.setflags(write=False)
    return out, carr


def same(got, carr, name, mode, ss):
    want, carr_want = case_reference(name, mode, ss)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(want)} bytes differ, the first at {int(np.flatnonzero(got != want)[0])}"
    assert carr.tobytes() == carr_want.tobytes(), (carr, carr_want)


def taken(fn):
    """fn() -> (its result, how many calls the device evaluation took meanwhile)"""
    before = gpsiq.device_eval_stats()[0]
    r = fn()
    return r, int(gpsiq.device_eval_stats()[0] - before)


# ---- the library's own decision ---------------------------------------------------------------------------------------------------
DEFAULT_CASES = [("edges", NCO_FIXED), ("edges", NCO_REFERENCE), ("one", NCO_FIXED), ("one", NCO_REFERENCE), ("short-ref", NCO_REFERENCE),
                 ("long-ref", NCO_REFERENCE)]


@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", DEFAULT_CASES)
def test_the_default_decision(ctx, monkeypatch, name, mode, kind, ss):
    """No GPSIQ_EVAL: the device path takes `long-ref` (48 blocks in GPSIQ_NCO_REFERENCE) and declines the others -- 47 blocks, one
    block, and 240 descriptors in the fixed model (fewer than 300 per host thread for any number of threads): the host path then
    reads rows that lie where the caller put them."""
    (got, carr), n = taken(lambda: render(ctx, dm.timeline(name), NS, FS, ss, mode, None, monkeypatch, kind))
    assert n == (1 if name == "long-ref" else 0), f"{name}: the device path took {n} calls"
    same(got, carr, name, mode, ss)


@pytest.mark.parametrize("ss", SIZES)
def test_short_ref_is_the_reference_itself(ctx, ref, monkeypatch, ss):
    """`short-ref` from device memory, the library's own decision (the host walker), against the reference's own loop (oracle/_ref)
    at the block length that loop has: fs / 10 samples.  A slot that ends unused hands out its last block's carr_phase."""
    fs = 2600000
    d = dm.timeline("short-ref")
    want, _, carr_ref = ref.run_blocks(d, fs, ss, SINK_IQFILE)
    (got, carr), n = taken(lambda: render(ctx, d, fs // 10, float(fs), ss, NCO_REFERENCE, None, monkeypatch, "device"))
    assert n == 0
    assert np.array_equal(got, want.view(np.uint8).reshape(-1))
    on = d["prn"][-1] > 0
    assert carr[on].tobytes() == carr_ref[-1][on].tobytes()
    assert (~on).any() and carr[~on].tobytes() == d["carr_phase"][-1][~on].tobytes()


# ---- GPSIQ_EVAL=host ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("to", ["host", "device-in-pieces"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["edges", "long-ref"])
def test_the_host_path_by_hand(ctx, monkeypatch, name, mode, kind, to, ss):
    """Into host memory in one piece, and into device memory with GPSIQ_PIECE_BLOCKS=8: the fixed model then takes its piece loop
    (test_the_piece_loop_cuts_where_a_satellite_changes reads the cuts), the reference model the walker's pieces."""
    if to != "host":
        monkeypatch.setenv("GPSIQ_PIECE_BLOCKS", "8")
    (got, carr), n = taken(lambda: render(ctx, dm.timeline(name), NS, FS, ss, mode, "host", monkeypatch, kind, to="host" if to == "host" else "device"))
    assert n == 0
    same(got, carr, name, mode, ss)


PIECES_CHILD = r'''
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.join(ROOT, "multi-sdr-gps-sim_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpsiq
import _desc_memory as dm
from gpsiq.abi import NCO_FIXED, SC08, SC16
os.environ["GPSIQ_EVAL"] = "host"
d = dm.timeline("edges")
nb, nc = d.shape
ctx = gpsiq.Context(0)
ctx.set_nco_mode(NCO_FIXED)
rows = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
for ss in (SC08, SC16):
    os.environ.pop("GPSIQ_PIECE_BLOCKS", None); os.environ.pop("GPSIQ_TRACE", None)
    want = ctx.generate_batch(d, dm.NSAMP, dm.FS, ss).view(np.uint8).reshape(-1)
    os.environ["GPSIQ_PIECE_BLOCKS"] = "8"; os.environ["GPSIQ_TRACE"] = "2"
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = gpsiq.device_eval_stats()[0]
    ctx.generate_batch((rows.data_ptr(), nb, nc), dm.NSAMP, dm.FS, ss, device_ptr=out.data_ptr())
    torch.cuda.synchronize()
    assert gpsiq.device_eval_stats()[0] == before
    assert np.array_equal(out.cpu().numpy(), want)
    print("same", ss)
ctx.close()
'''


def test_the_piece_loop_cuts_where_a_satellite_changes():
    """GPSIQ_EVAL=host, fixed model, device-resident `edges` into device memory under GPSIQ_PIECE_BLOCKS=8: GPSIQ_TRACE=2 (read per
    call, written to stderr: a child process) shows the piece loop of generate_batch() cutting [0, 1, 3, 7, 16, 32, 40) -- the first
    piece is an eighth of the knob, each later one 2.2 times the one before (piece_ends, csrc/gpsiq_pieces.h).  No value of the
    knob cuts 40 blocks at block 8 (2 n <= 40 leaves first pieces of 1 or 2 blocks, and both plans pass 7 -> 16); 8 puts a cut on
    the slot's SECOND change of satellite, at block 16, where the loop reads ch[16 * nchan + i] to learn that the slot seeds again."""
    import re
    r = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + PIECES_CHILD], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["same", str(SC08), "same", str(SC16)], (r.stdout + r.stderr)[-3000:]
    cuts = [(int(a), int(b)) for a, b in re.findall(r"piece \d+, blocks \[(\d+), (\d+)\): quantise", r.stderr)]
    per_call = len(cuts) // 2
    assert per_call > 1 and cuts[:per_call] == cuts[per_call:], r.stderr[-3000:]            # one call per sample size
    cuts = cuts[:per_call]
    assert cuts[0][0] == 0 and cuts[-1][1] == dm.NB_EDGES and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])), cuts
    assert dm.CHANGE_AT[1] in [a for a, _ in cuts], cuts


# ---- GPSIQ_CHAIN ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("chain", ["device", "host"])
def test_the_chain_by_hand(ctx, monkeypatch, chain, kind, ss):
    """GPSIQ_CHAIN asks for the host evaluation (the device path declines, 48 blocks or not); with `device` the chain's inputs are
    cut out of ch on the host pool (gpsiq_chain_stage_inputs)"""
    monkeypatch.setenv("GPSIQ_CHAIN", chain)
    (got, carr), n = taken(lambda: render(ctx, dm.timeline("long-ref"), NS, FS, ss, NCO_REFERENCE, None, monkeypatch, kind))
    assert n == 0
    same(got, carr, "long-ref", NCO_REFERENCE, ss)


# ---- GPSIQ_EVAL=device at the small shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["edges", "one"])
def test_the_device_path_where_the_first_block_is_the_last(ctx, monkeypatch, name, mode, kind, ss):
    (got, carr), n = taken(lambda: render(ctx, dm.timeline(name), NS, FS, ss, mode, "device", monkeypatch, kind))
    assert n == 1
    same(got, carr, name, mode, ss)


# ---- continuation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["host", "device"])
def test_a_call_continued_from_rows_in_that_memory(ctx, monkeypatch, how, mode, kind, ss):
    """`edges` in two calls cut at block 20: block 0 of the second carries what the first handed out, written into the rows before
    they go to page-locked / device memory.  The same bytes and the same carr_out as one call."""
    d = dm.timeline("edges")
    (a, carr), n1 = taken(lambda: render(ctx, d[:dm.CUT], NS, FS, ss, mode, how, monkeypatch, kind))
    d2 = d[dm.CUT:].copy()
    d2["carr_phase"][0] = carr
    (b, carr2), n2 = taken(lambda: render(ctx, d2, NS, FS, ss, mode, how, monkeypatch, kind))
    assert (n1, n2) == ((1, 1) if how == "device" else (0, 0))
    same(np.concatenate([a, b]), carr2, "edges", mode, ss)


# ---- a refused descriptor --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["host", "device"])
def test_a_refused_descriptor_reads_the_same_from_every_memory(ctx, monkeypatch, how, mode, ss):
    """Between the two halves of a continued `edges` the whole of `refused` is rendered and fails: the code and the host quantiser's
    words for block 30 are the same whichever memory holds the rows (the device path fetches the row back for them), and the second
    half then continues as if the failed call had not been -- the carried phases were untouched."""
    d, bad = dm.timeline("edges"), dm.timeline("refused")
    said = {}
    for kind in ["pageable"] + KINDS:
        a, carr = render(ctx, d[:dm.CUT], NS, FS, ss, mode, how, monkeypatch, "pageable")
        with pytest.raises(gpsiq.GpsiqError, match="block 30.*f_code") as err:
            render(ctx, bad, NS, FS, ss, mode, how, monkeypatch, kind)
        said[kind] = (err.value.code, str(err.value))
        d2 = d[dm.CUT:].copy()
        d2["carr_phase"][0] = carr
        b, carr2 = render(ctx, d2, NS, FS, ss, mode, how, monkeypatch, kind)
        same(np.concatenate([a, b]), carr2, "edges", mode, ss)
    assert said["pageable"][0] == -2 and said["pinned"] == said["pageable"] and said["device"] == said["pageable"], said


# ---- pointers that must be refused ---------------------------------------------------------------------------------------------------
def on_device(d, device="cuda"):
    import torch
    return torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).to(device)


def refused_pointer(call, words="device memory"):
    """call() fails with GPSIQ_E_ARG before anything happened: the words name the kind of pointer, the device path saw nothing"""
    stats = gpsiq.device_eval_stats()
    with pytest.raises(gpsiq.GpsiqError, match=words) as err:
        gpsiq._check(call())
    assert err.value.code == -1, err.value
    assert np.array_equal(gpsiq.device_eval_stats(), stats)


@pytest.mark.parametrize("how", ["host", "device"])
def test_generate_seeded_refuses_descriptors_in_device_memory(ctx, monkeypatch, how):
    d = dm.timeline("edges")
    nb, nc = d.shape
    starts, _, _ = gpsiq.reference_chain(gpsiq.chain_inputs(d), FS, NS)
    monkeypatch.setenv("GPSIQ_EVAL", how)
    ctx.set_nco_mode(NCO_REFERENCE)
    rows = on_device(d)
    out = np.zeros(nb * 2 * NS, dtype=np.int8)
    refused_pointer(lambda: gpsiq._generate_seeded(ctx._h, gpsiq._vp(rows.data_ptr()), nb, nc, NS, FS, SC08, gpsiq._p(starts), gpsiq._p(out), 0),
                    "gpsiq_generate_seeded.*device memory")
    assert not out.any()
    got = ctx.generate_seeded(d, NS, FS, SC08, starts)
    assert np.array_equal(got.view(np.uint8).reshape(-1), case_reference("edges", NCO_REFERENCE, SC08)[0])


@pytest.mark.parametrize("mode", MODES)
def test_generate_batch_multi_refuses_descriptors_in_device_memory(ctx, mode):
    import ctypes as C
    d = dm.timeline("edges")
    nb, nc = d.shape
    ctx.set_nco_mode(mode)
    rows = on_device(d)
    out = np.zeros(nb * 2 * NS, dtype=np.int8)
    carr = np.full(nc, -1.0)
    handles = (C.c_void_p * 1)(ctx._h)
    refused_pointer(lambda: gpsiq._generate_batch_multi(handles, 1, gpsiq._vp(rows.data_ptr()), nb, nc, NS, FS, SC08, gpsiq._p(out), None, gpsiq._p(carr)),
                    "gpsiq_generate_batch_multi.*device memory")
    assert not out.any() and (carr == -1.0).all()
    got = gpsiq.generate_batch_multi([ctx], d, NS, FS, SC08, carr_out=carr)
    same(got.view(np.uint8).reshape(-1), carr, "edges", mode, SC08)


@pytest.mark.parametrize("mode", MODES)
def test_generate_batch_packed_refuses_descriptors_in_device_memory(ctx, monkeypatch, mode):
    d = dm.timeline("edges")
    nb, nc = d.shape
    ctx.set_nco_mode(mode)
    ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(d["gain"][0], 0.0), 7 / 3.0), 7)
    rows = on_device(d)
    plen = pr.packed_block_bytes(NS, pr.PK4)
    out = np.zeros(nb * plen, dtype=np.uint8)
    carr = np.full(nc, -1.0)
    refused_pointer(lambda: gpsiq._generate_batch_packed(ctx._h, gpsiq._vp(rows.data_ptr()), nb, nc, NS, FS, pr.PK4, gpsiq._p(out), plen, gpsiq._p(carr)),
                    "gpsiq_generate_batch_packed.*device memory")
    assert not out.any() and (carr == -1.0).all()
    got = ctx.generate_batch_packed(d, NS, FS, pr.PK4, carr_out=carr)
    monkeypatch.setenv("GPSIQ_EVAL", "host")
    ctx2 = gpsiq.Context(0)
    try:
        ctx2.set_nco_mode(mode)
        ctx2.set_level(gpsiq.level_mult(gpsiq.composite_rms(d["gain"][0], 0.0), 7 / 3.0), 7)
        carr_want = np.zeros(nc)
        want, clamped = pr.pack(ctx2.generate_batch(d, NS, FS, SC08, carr_out=carr_want), pr.PK4)
    finally:
        ctx2.close()
    assert clamped == 0 and np.array_equal(got, want) and carr.tobytes() == carr_want.tobytes()


def test_descriptors_on_another_device_are_refused(ctx, monkeypatch):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: descriptors in another device's memory need two")
    d = dm.timeline("edges")
    nb, nc = d.shape
    rows = on_device(d, "cuda:1")
    out = np.zeros(nb * 2 * NS, dtype=np.int8)
    carr = np.full(nc, -1.0)
    for how in ("host", "device"):
        monkeypatch.setenv("GPSIQ_EVAL", how)
        refused_pointer(lambda: gpsiq._generate_batch(ctx._h, gpsiq._vp(rows.data_ptr()), nb, nc, NS, FS, SC08, gpsiq._p(out), 0, gpsiq._p(carr)),
                        "device memory of device 1, the context is on device 0")
        assert not out.any() and (carr == -1.0).all()
    got, carr = render(ctx, d, NS, FS, SC08, NCO_FIXED, "host", monkeypatch, "device")
    same(got, carr, "edges", NCO_FIXED, SC08)


# ---- a base that is 8-byte aligned and no more -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ss", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("how", ["host", "device"])
def test_rows_eight_bytes_into_a_device_allocation(ctx, monkeypatch, how, mode, ss):
    """gpsiq_chan_t is 8-byte aligned: neither the copy down to the host path nor the device's pack may ask for more"""
    (got, carr), n = taken(lambda: render(ctx, dm.timeline("edges"), NS, FS, ss, mode, how, monkeypatch, "device", offset=8))
    assert n == (1 if how == "device" else 0)
    same(got, carr, "edges", mode, ss)
