"""One long-lived context through every rendering path at a small size, then at a size that makes the path's growable buffers
grow, then at the small size again: every output is, byte for byte (and every carried phase, bit for bit), what a FRESH context
renders for the same call.  The context's members own their resources (csrc/gpsiq_own.h) and every buffer grows through one
reserve(); what this test holds is that a buffer which was small, grew and is then used small again serves the same bytes as one
made at the right size.  Device memory is not measured (it is device-wide on a shared machine): leaks, double frees and the
recovery from failed allocations are tests/test_own_types.py's, on the CPU.

Sizes.  Batch paths: 4 channels, 1024 samples per block, 2 blocks, then 160, then 2.  After the first round the exact-capacity
buffers (a set's descriptors and their staging: n = blocks x channels; the output staging: 2048- or 4096-byte rows x blocks;
segm's scratch) hold 8 descriptors / 2 rows, and the chain's and the device evaluation's rows hold n + n/4 + 256 = 266
block-channels; the raw and the seed rows n + n/4 + 16 = 26.  160 x 4 = 640 exceeds every one of them.  Channel 0 runs at a
Doppler of exactly fs/3 from phase 0: its double accumulator lands on a table boundary every third sample, and the reference
model then needs ~341 patches per block -- 682 in round one (more than the 256 a patch list starts with), ~54 600 in round two
(below the 65 536 the device evaluation's lists hold), so a set's patch list and its staging grow as well.
Block calls: the growable buffers are the slot's output row and its patch list, so the rounds are 256, 4096 and 256 samples:
~86, ~1366 and ~86 patches (256 entries first, regrown in round two), rows of 512 / 1024 bytes, then 8192 / 16384.
Not forced to grow here, because what sizes them is decided by the data on the device and not by the call: the repair columns
(a slot whose certified map does not apply) and the host walker's descriptors; tests/test_gpu_device_eval.py exercises both
at one size, the CPU test their growth.

Between compared calls the carrier continuation is reset by toggling the NCO mode and next_block is set explicitly, so that
the long-lived and the fresh context start from the same state.  GPSIQ_EVAL is read per call: the host path is pinned in this
process, the device path in a child process of its own (one, run under its own time limit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "multi-sdr-gps-sim_amd"), os.path.join(_root, "tests")]

import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, SC08, SC16
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

FS, NC, NS = 2.6e6, 4, 1024
ROUNDS = (2, 160, 2)
BLOCK_ROUNDS = (256, 4096, 256)


def timeline(nb, seed):
    d = synth_blocks(nb, NC, seed=seed)
    d["f_carr"][:, 0] = FS / 3.0                     # exactly a third of a cycle per sample, from phase 0: patches (see above)
    d["f_code"][:, 0] = 1.023e6 + d["f_carr"][:, 0] / 1540.0
    d["carr_phase"][:, 0] = 0.0
    return d


def reset(ctx, mode, next_block=0):
    """The state a compared call starts from: no carrier continuation, the mode, noise off, the block counter."""
    ctx.set_nco_mode(NCO_REFERENCE if mode == NCO_FIXED else NCO_FIXED)
    ctx.set_nco_mode(mode)
    ctx.set_noise(0, 0.0, next_block)


def same_as_fresh(long_lived, call, mode, next_block=0):
    """call(ctx) -> a tuple of arrays; on the long-lived context and on a fresh one."""
    reset(long_lived, mode, next_block)
    got = call(long_lived)
    fresh = gpsiq.Context(0)
    try:
        reset(fresh, mode, next_block)
        want = call(fresh)
    finally:
        fresh.close()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
    return got


@pytest.fixture()
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE])
@pytest.mark.parametrize("ss", [SC08, SC16])
def test_block_calls_small_large_small(ctx, mode, ss):
    import torch
    d = timeline(3, 41)
    for k, ns in enumerate(BLOCK_ROUNDS):
        if mode == NCO_REFERENCE:
            npatch = len(gpsiq.reference_blocks(d[k:k + 1], FS, ns)[1])
            assert (npatch > 256) == (ns == BLOCK_ROUNDS[1]) and npatch > 0      # the patch list: 256 entries, regrown, used small again
        same_as_fresh(ctx, lambda c: c.generate_block(d[k], ns, FS, ss), mode, next_block=k)

        def queued(c):
            # three blocks in flight on the ring of slots, then the wait
            bufs = [torch.zeros(2 * ns * ss, dtype=torch.uint8).pin_memory() for _ in range(3)]
            carr = [c.generate_block_async(d[j], ns, FS, ss, bufs[j].data_ptr()) for j in range(3)]
            c.wait()
            return tuple(b.numpy().copy() for b in bufs) + tuple(carr)
        same_as_fresh(ctx, queued, mode, next_block=k)


def batch_rounds(ctx, device_path):
    """generate_batch (both models) and generate_seeded, to a host destination and to a misaligned device destination."""
    import torch
    for mode, seeded in ((NCO_FIXED, False), (NCO_REFERENCE, False), (NCO_REFERENCE, True)):
        for ss in (SC08, SC16):
            for nb in ROUNDS:
                d = timeline(nb, 100 + nb)
                starts = gpsiq.reference_chain(gpsiq.chain_inputs(d), FS, NS)[0] if seeded else None
                dev = torch.zeros(nb * 2 * NS * ss + 16, dtype=torch.uint8, device="cuda")

                def to_host(c):
                    carr = np.zeros(NC)
                    if seeded:
                        return (c.generate_seeded(d, NS, FS, ss, starts),)
                    return c.generate_batch(d, NS, FS, ss, carr_out=carr), carr

                def to_device(c, pinned=False):
                    # one element off the allocation's alignment, so not 4-byte aligned: the call cannot render in place, it renders
                    # into the context's staging and copies across
                    dev.zero_()
                    carr = np.zeros(NC)
                    src, keep = d, None
                    if pinned:
                        keep = torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).pin_memory()
                        src = (keep.data_ptr(), nb, NC)
                    if seeded:
                        c.generate_seeded(d, NS, FS, ss, starts, device_ptr=dev.data_ptr() + ss)
                    else:
                        c.generate_batch(src, NS, FS, ss, device_ptr=dev.data_ptr() + ss, carr_out=carr)
                    torch.cuda.synchronize()
                    return dev.cpu().numpy(), carr

                before = gpsiq.device_eval_stats()
                host_out = same_as_fresh(ctx, to_host, mode)[0]
                dev_out = same_as_fresh(ctx, to_device, mode)[0]
                assert dev_out[ss:ss + host_out.nbytes].tobytes() == host_out.tobytes()
                calls = 4
                if device_path and not seeded:                       # page-locked descriptors: the raw rows in device memory grow too
                    same_as_fresh(ctx, lambda c: to_device(c, True), mode)
                    calls += 2
                after = gpsiq.device_eval_stats()
                assert after[0] - before[0] == (calls if device_path else 0), "the calls did not take the path under test"
                assert after[5] == before[5], "a device evaluation fell back to the host path: the patch lists overflowed"


def test_batch_calls_small_large_small_host_path(ctx, monkeypatch):
    monkeypatch.setenv("GPSIQ_EVAL", "host")
    batch_rounds(ctx, False)


def test_batch_calls_small_large_small_device_path():
    env = dict(os.environ, GPSIQ_EVAL="device")
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.splitlines()[-1] == "ok"


def test_resident_set_patches_and_segm_launch(ctx):
    """set_descriptors + set_patches + launch with segm, the variant that works in the context's scratch."""
    import torch
    segm = gpsiq.variants()["segm"]
    for ss in (SC08, SC16):
        for nb in ROUNDS:
            q, patches, _ = gpsiq.reference_blocks(timeline(nb, 300 + nb), FS, NS)
            assert len(patches) > 256
            out = torch.zeros(nb * 2 * NS * ss, dtype=torch.uint8, device="cuda")

            def launched(c):
                out.zero_()
                c.set_descriptors(q)
                c.set_patches(patches)
                c.launch(0, nb, NS, ss, out.data_ptr(), 2 * NS * ss, variant=segm)
                c.synchronize()
                return (out.cpu().numpy(),)
            same_as_fresh(ctx, launched, NCO_REFERENCE)


def test_two_contexts_keep_their_own_noise_and_level():
    """generate_batch_multi renders every range with context 0's noise and level and gives the other context its own back: after
    every round both contexts' noise states are their own (context 0 moved on by the call's blocks), and at the end each renders
    what a fresh context with its own settings renders (context 1: its own noise, no level)."""
    own = [dict(seed=5, sigma=40.0, mult=30000, qmax=100), dict(seed=9, sigma=25.0, mult=0, qmax=0)]

    def configured():
        cs = [gpsiq.Context(0), gpsiq.Context(0)]
        cs[0].set_level(own[0]["mult"], own[0]["qmax"])          # a level on context 0 only
        return cs

    def multi(cs, d):
        for c, o, first in zip(cs, own, (1000, 7)):
            c.set_nco_mode(NCO_REFERENCE)
            c.set_nco_mode(NCO_FIXED)
            c.set_noise(o["seed"], o["sigma"], first)
        return gpsiq.generate_batch_multi(cs, d, NS, FS, SC08)
    pair = configured()
    try:
        for nb in ROUNDS:
            d = timeline(nb, 77)
            got = multi(pair, d)
            fresh = configured()
            try:
                want = multi(fresh, d)
            finally:
                for c in fresh:
                    c.close()
            assert got.tobytes() == want.tobytes()
            assert pair[0].noise_state() == (own[0]["seed"], own[0]["sigma"], 1000 + nb)
            assert pair[1].noise_state() == (own[1]["seed"], own[1]["sigma"], 7)
        d = timeline(3, 78)
        for c, o in zip(pair, own):
            f = gpsiq.Context(0)
            try:
                f.set_noise(o["seed"], o["sigma"], 50)
                if o["mult"]:
                    f.set_level(o["mult"], o["qmax"])
                seed, sigma, _ = c.noise_state()                  # as the call left them; only the counter is set
                c.set_noise(seed, sigma, 50)
                c.set_nco_mode(NCO_REFERENCE)
                c.set_nco_mode(NCO_FIXED)
                assert c.generate_batch(d, NS, FS, SC08).tobytes() == f.generate_batch(d, NS, FS, SC08).tobytes()
            finally:
                f.close()
    finally:
        for c in pair:
            c.close()


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available() and os.environ.get("GPSIQ_EVAL") == "device"
    c = gpsiq.Context(0)
    try:
        batch_rounds(c, True)
    finally:
        c.close()
    print("ok")
