"""gpsiq_generate_batch_agc on the MI355X: byte for byte, count for count, state for state and carrier phase bit for bit gpsiq_agc of what
ONE gpsiq_generate_batch over the whole timeline writes on a second context -- 7 blocks of 1 000 samples (not a multiple of any window),
4 channels, noise and level on -- in pieces of 1, 2 and 3 blocks and whole, in both NCO models; with a window shorter and a window
longer than a block, a hold longer than a block under a threshold that a few samples of the stream exceed, from a fresh and from a given
state; a state handed from one call to the next against one call over both; against tests/_agc_ref.py's restatement and, through
tests/test_gpu_agc.py's check, against the device call itself; the refusals, and gpsiq_runahead --agc.  Run with -m gpu."""
import numpy as np
import pytest

import _agc_ref as ar
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks
from test_gpu_agc import check

pytestmark = pytest.mark.gpu

GUARD = 0x7F
FS, NB, NSAMP, NC = 10.4e6, 7, 1000, 4


def descriptors(seed, nb=NB, nc=NC):
    """a satellite change on a piece edge (block 3 with pieces of 3) and an unused slot"""
    d = synth_blocks(nb, nc, seed=seed)
    d["prn"][3:, 1] = 29
    d["carr_phase"][3:, 1] = 0.3125
    d["prn"][:, 2] = 0
    return d


def settings(c, mode, ss):
    sigma = gpsiq.noise_sigma_for_cn0(50.0, 1.0, FS)
    c.set_nco_mode(mode)
    c.set_noise(77, sigma, 5)
    q = 127 if ss == SC08 else 32767
    c.set_level(gpsiq.level_mult(gpsiq.composite_rms(np.full(3, 0.6), sigma), q / 4.0), q)


def threshold_few_exceed(stream):
    """the largest threshold that some sample exceeds: the second largest of the samples' peak elements.  The samples that hold the
    largest one exceed it -- a few where the level stage has clamped to it, one otherwise"""
    peaks = np.unique(np.abs(stream.astype(np.int32)).max(axis=1))
    assert len(peaks) >= 2
    return int(peaks[-2])


def configs(stream, ss):
    """(cfg, out_sample_size, state): a window shorter than a block into the narrow quantiser from a fresh stream; a window and a hold
    longer than a block, a few samples above the threshold, from a state with a window in progress, a ring and a hold"""
    t = threshold_few_exceed(stream)
    a = ar.cfg(window=192, navg=2, target_q8=int(256 * 2.5), mult0=65536, blank_thresh=0, blank_hold=0, qmax=7)
    b = ar.cfg(window=1088, navg=3, target_q8=256 * (40 if ss == SC08 else 9000), mult0=30000, blank_thresh=t, blank_hold=1024, qmax=127 if ss == SC08 else 32767)
    top = 40 * 40 if ss == SC08 else 9000 * 9000
    given = ar.State(((2 * 1088 * top, 2 * 1088),), 700 * top, 700, 353, 100)
    return (a, SC08, ar.FRESH), (b, ss, given)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE], ids=["fixed", "reference"])
@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
def test_batch_agc_is_the_stage_of_one_batch_call(ctx_pair, mode, ss, monkeypatch):
    a, b = ctx_pair
    settings(a, mode, ss)
    settings(b, mode, ss)
    d = descriptors(820 + ss)
    carr_a, carr_b = np.zeros(NC), np.zeros(NC)
    stream = b.generate_batch(d, NSAMP, FS, ss, carr_out=carr_b).reshape(-1, 2)
    for c, oss, start in configs(stream, ss):
        want = check(b, stream, c, start, oss)                       # the restatement, and the device call itself on the same stream
        if c.blank_thresh:
            assert (np.abs(stream.astype(np.int32)).max(axis=1) > c.blank_thresh).any() and 100 < want[2] < NB * NSAMP                      # more than the hold handed in alone
        else:
            assert want[1] > 0
        row = 2 * NSAMP * oss
        for piece, pieces in (("1", 7), ("2", 4), ("3", 3), (None, 1)):
            if piece is None:
                monkeypatch.delenv("GPSIQ_AGC_PIECE_BLOCKS")
            else:
                monkeypatch.setenv("GPSIQ_AGC_PIECE_BLOCKS", piece)
            settings(a, mode, ss)                                    # the noise block counter back to 5
            stride = row + (16 if piece == "2" else 0)               # once with room between the blocks
            host = np.full(NB * stride + 64, GUARD, dtype=np.uint8)
            st = ar.to_lib_state(start)
            _, clipped, blanked = a.generate_batch_agc(d, NSAMP, FS, ss, ar.to_lib_cfg(c), oss, state=st, host_ptr=host.ctypes.data, block_stride=stride,
                                                       carr_out=carr_a)
            assert a.agc_last_plan()[5] == pieces
            blocks = host[:NB * stride].reshape(NB, stride)
            got = np.ascontiguousarray(blocks[:, :row]).view(want[0].dtype).reshape(-1, 2)
            assert np.array_equal(got, want[0]), (piece, np.argwhere(got != want[0])[:4])
            assert (blocks[:, row:] == GUARD).all() and (host[NB * stride:] == GUARD).all()
            assert (clipped, blanked) == want[1:3] and ar.from_lib_state(st) == want[4], piece
            assert carr_a.tobytes() == carr_b.tobytes()
        assert a.noise_state() == b.noise_state()


@pytest.fixture(scope="module")
def ctx_pair():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    yield a, b
    a.close()
    b.close()


def test_a_state_handed_from_one_call_to_the_next(ctx_pair, monkeypatch):
    """two calls of 3 and 4 blocks, the second from the state, the phases and the noise counter the first left, against gpsiq_agc over
    both calls' streams in one span; a fresh state through NULL and a page-locked destination"""
    import torch
    a, b = ctx_pair
    monkeypatch.setenv("GPSIQ_AGC_PIECE_BLOCKS", "2")
    for c in (a, b):
        settings(c, NCO_FIXED, SC16)
    d = descriptors(831)
    carr = np.zeros(NC)
    first = b.generate_batch(d[:3], NSAMP, FS, SC16, carr_out=carr).reshape(-1, 2)
    d2 = d[3:].copy()
    keep = (d2["prn"][0] > 0) & (d2["prn"][0] == d["prn"][2])
    d2["carr_phase"][0, keep] = carr[keep]
    second = b.generate_batch(d2, NSAMP, FS, SC16).reshape(-1, 2)
    stream = np.concatenate([first, second])
    c = ar.cfg(window=1088, navg=2, target_q8=256 * 30, mult0=200, blank_thresh=threshold_few_exceed(stream), blank_hold=700, qmax=127)
    want = check(b, stream, c, ar.FRESH, SC08)
    st = gpsiq.AgcState()
    got1, cl1, bl1 = a.generate_batch_agc(d[:3], NSAMP, FS, SC16, ar.to_lib_cfg(c), SC08, state=st, carr_out=carr)
    assert ar.from_lib_state(st) == ar.agc_ref(first, c, ar.FRESH, SC08)[4]
    pinned = torch.full((4 * 2 * NSAMP + 64,), GUARD, dtype=torch.uint8).pin_memory()
    _, cl2, bl2 = a.generate_batch_agc(d2, NSAMP, FS, SC16, ar.to_lib_cfg(c), SC08, state=st, host_ptr=pinned.data_ptr())
    got2 = pinned.numpy()
    assert np.array_equal(got1.reshape(-1, 2), want[0][:3 * NSAMP]) and np.array_equal(got2[:8 * NSAMP].view(np.int8).reshape(-1, 2), want[0][3 * NSAMP:])
    assert (got2[8 * NSAMP:] == GUARD).all() and (cl1 + cl2, bl1 + bl2) == want[1:3] and ar.from_lib_state(st) == want[4]
    assert a.noise_state() == b.noise_state()
    # state NULL: a fresh stream, nothing returned
    for ctx in (a, b):
        settings(ctx, NCO_FIXED, SC16)
    got, cl, bl = a.generate_batch_agc(d[:3], NSAMP, FS, SC16, ar.to_lib_cfg(c), SC08)
    assert np.array_equal(got, got1) and (cl, bl) == (cl1, bl1)


def test_refusals_and_empty_batches(ctx_pair, monkeypatch):
    import torch
    a, b = ctx_pair
    monkeypatch.delenv("GPSIQ_AGC_PIECE_BLOCKS", raising=False)
    for c in (a, b):
        settings(c, NCO_FIXED, SC08)
    d = descriptors(840)
    good = ar.cfg(window=64, navg=2, target_q8=256 * 30, blank_thresh=100, blank_hold=8, qmax=127)
    for bad in (dict(window=100), dict(navg=0), dict(target_q8=0), dict(mult_min=0), dict(mult0=1 << 24), dict(blank_thresh=-1), dict(blank_hold=1025),
                dict(qmax=128), dict(qmax=0)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_agc(d, NSAMP, FS, SC08, ar.to_lib_cfg(good._replace(**bad)), SC08)
        assert e.value.code == -1, bad
    for st in (ar.State(((5, 2), (6, 2), (7, 2)), 0, 0, 0, 0), ar.State((), 0, 0, 64, 0), ar.State((), 0, 4, 1, 0), ar.State((), 0, 0, 0, 9)):
        with pytest.raises(gpsiq.GpsiqError) as e:
            a.generate_batch_agc(d, NSAMP, FS, SC08, ar.to_lib_cfg(good), SC08, state=ar.to_lib_state(st))
        assert e.value.code == -1, st
    with pytest.raises(gpsiq.GpsiqError) as e:                         # a stride shorter than a block of outputs
        a.generate_batch_agc(d, NSAMP, FS, SC08, ar.to_lib_cfg(good), SC16, host_ptr=np.zeros(NB * 4 * NSAMP, np.uint8).ctypes.data, block_stride=4 * NSAMP - 4)
    assert e.value.code == -1
    # descriptors in device memory: the pieces' first rows are rewritten on the host
    dev = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).cuda()
    out = np.zeros(NB * 2 * NSAMP, np.uint8)
    cfg = ar.to_lib_cfg(good)
    assert gpsiq._generate_batch_agc(a._h, dev.data_ptr(), NB, NC, NSAMP, FS, SC08, gpsiq.C.byref(cfg), None, SC08, gpsiq._p(out), 2 * NSAMP, None, None, None) == -1
    assert a.noise_state() == b.noise_state()                        # nothing was rendered by any of these
    # an empty batch and blocks of no samples: counts of 0, the state as it was
    st = ar.to_lib_state(ar.State(((5, 2),), 9, 2, 63, 8))
    before = st.as_tuple()
    assert a.generate_batch_agc(d[:0], NSAMP, FS, SC08, cfg, SC08, state=st)[1:] == (0, 0) and st.as_tuple() == before
    assert a.generate_batch_agc(d, 0, FS, SC08, cfg, SC08, state=st)[1:] == (0, 0) and st.as_tuple() == before
    # a used context called again with more blocks, more samples and wider elements: grow-only buffers
    for c in (a, b):
        settings(c, NCO_FIXED, SC16)
    big = descriptors(841, 9)
    stream = b.generate_batch(big, 3 * NSAMP + 8, FS, SC16).reshape(-1, 2)
    c2 = ar.cfg(window=64, navg=64, target_q8=256 * 5000, blank_thresh=threshold_few_exceed(stream), blank_hold=65, qmax=32767)
    want = ar.agc_ref(stream, c2, ar.FRESH, SC16)
    got, cl, bl = a.generate_batch_agc(big, 3 * NSAMP + 8, FS, SC16, ar.to_lib_cfg(c2), SC16)
    assert np.array_equal(got.reshape(-1, 2), want[0]) and (cl, bl) == want[1:3]


def test_runahead_agc_flag(tmp_path, monkeypatch):
    """gpsiq_runahead --agc writes gpsiq_agc of the file the same flags write without it, the state running on from call to call of the
    library -- here one call of three blocks in two pieces -- and prints both counts and the multipliers"""
    import os
    import subprocess
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    monkeypatch.setenv("GPSIQ_AGC_PIECE_BLOCKS", "2")
    fs, nblocks, nchan = 2.6e6, 3, 8
    ns = int(np.floor(fs / 10.0 + 0.5))
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))
    flags = ("--cn0", "45", "--seed", "7", "--level", "9000")

    def run(*more):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), "2", out, *flags, *more], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.int16), r.stdout
    plain, _ = run()
    assert plain.size == nblocks * 2 * ns
    stream = plain.reshape(-1, 2)
    t = threshold_few_exceed(stream)
    got, text = run("--agc", "0.9,1,4096,4", "--blank", f"{t},300")
    c = ar.cfg(window=4096, navg=4, target_q8=230, mult0=65536, mult_min=1, mult_max=(1 << 24) - 1, blank_thresh=t, blank_hold=300, qmax=1)
    want = ar.agc_ref(stream, c, ar.FRESH, SC16)
    assert got.size == plain.size and np.array_equal(got.reshape(-1, 2), want[0])
    ring = want[4].ring
    last = ar.mult(c, sum(s for s, _ in ring), sum(k for _, k in ring))
    assert f"{want[1]} elements clipped, {want[2]} samples blanked, multiplier 65536 at the first window, {last} at the end" in text
    assert want[2] >= 301 and last < 65536
