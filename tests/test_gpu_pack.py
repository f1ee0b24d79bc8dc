"""gpsiq_pack, gpsiq_unpack and gpsiq_generate_batch_packed on the MI355X: every output byte, every guard byte and every count equals
tests/_pack_ref.py's restatement of the contract (include/gpsiq_rows.h, "Packed streams").  The sources are random bytes unless
stated -- the kernels are pure functions of the stream -- between guard bytes of 0x7f that must neither enter nor change.
Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _pack_ref as pr
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, PK2, PK4, SC08, SC16, elem_dtype
from gpsiq.scenario import synth_blocks

pytestmark = pytest.mark.gpu

GUARD = 0x7F
# one element, odd lengths (2 bits: a half-used last byte), both sides of a 16-byte lane, of a wave and of a workgroup, a ragged length
NSAMP = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4095, 70001]
NBLOCKS = [1, 2, 5]
FORMATS = [(ss, bits) for ss in (SC08, SC16) for bits in (PK4, PK2)]
TAIL = 64            # guard bytes behind the last block of a destination


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """random bytes every case cuts its source from (computed once, never written)"""
    a = np.random.default_rng(2024).integers(0, 256, size=5 * 4 * 70001 + 4096, dtype=np.uint8)
    a.setflags(write=False)
    return a


def up4(n):
    return (n + 3) & ~3


def rows(blocks, stride, tail=0):
    """blocks: uint8 [nblocks][len] -> uint8 [nblocks * stride + tail], 0x7f wherever no block byte lies"""
    buf = np.full(len(blocks) * stride + tail, GUARD, dtype=np.uint8)
    v = buf[:len(blocks) * stride].reshape(len(blocks), stride)
    v[:, :blocks.shape[1]] = blocks
    return buf


def run_pack(ctx, x, ss, bits, src_stride, dst_stride):
    """x: elements [nblocks][2 * nsamp] -> (packed uint8 [nblocks][plen] as the device wrote it, count); guards compared"""
    import torch
    nb, nsamp = x.shape[0], x.shape[1] // 2
    plen = pr.packed_block_bytes(nsamp, bits)
    src = torch.from_numpy(rows(np.ascontiguousarray(x).view(np.uint8).reshape(nb, -1), src_stride)).cuda()
    before = np.full(nb * dst_stride + TAIL, GUARD, dtype=np.uint8)
    dst = torch.from_numpy(before).cuda()
    clipped, ms = ctx.pack(nb, nsamp, ss, src.data_ptr(), src_stride, bits, dst.data_ptr(), dst_stride)
    got = dst.cpu().numpy()
    body = got[:nb * dst_stride].reshape(nb, dst_stride)
    assert (body[:, plen:] == GUARD).all() and (got[nb * dst_stride:] == GUARD).all(), "guard bytes of the destination changed"
    assert ms >= 0.0
    return body[:, :plen], clipped


def run_unpack(ctx, p, nsamp, bits, ss, src_stride, dst_stride):
    import torch
    nb = p.shape[0]
    src = torch.from_numpy(rows(p, src_stride)).cuda()
    dst = torch.from_numpy(np.full(nb * dst_stride + TAIL, GUARD, dtype=np.uint8)).cuda()
    ms = ctx.unpack(nb, nsamp, bits, src.data_ptr(), src_stride, ss, dst.data_ptr(), dst_stride)
    got = dst.cpu().numpy()
    body = got[:nb * dst_stride].reshape(nb, dst_stride)
    blen = 2 * nsamp * ss
    assert (body[:, blen:] == GUARD).all() and (got[nb * dst_stride:] == GUARD).all(), "guard bytes of the destination changed"
    assert ms >= 0.0
    return np.ascontiguousarray(body[:, :blen]).view(elem_dtype(ss))


def shapes():
    """(nsamp, nblocks, source stride offset, destination stride offset): the full cross -- every length with every block count, with
    source strides that put block bases at 0, 4, 8 and 12 modulo 16, and with both destination strides"""
    return [(n, nb, s, d) for n in NSAMP for nb in NBLOCKS for s in (0, 4, 20) for d in (0, 4)]


@pytest.mark.parametrize("ss,bits", FORMATS, ids=lambda v: str(v))
def test_pack_every_shape(ctx, pool, ss, bits):
    for n, nb, ds, dd in shapes():
        blen = 2 * n * ss
        x = pool[n % 1000:n % 1000 + nb * blen].reshape(nb, blen).view(elem_dtype(ss))
        want, count = pr.pack(x, bits)
        got, clipped = run_pack(ctx, x, ss, bits, up4(blen) + ds, up4(want.shape[1]) + dd)
        assert np.array_equal(got, want), (n, nb, ds, dd, np.argwhere(got != want)[:4])
        assert clipped == count, (n, nb, ds, dd, clipped, count)       # the reference's: no guard byte of the source entered


@pytest.mark.parametrize("ss,bits", FORMATS, ids=lambda v: str(v))
def test_unpack_every_shape(ctx, pool, ss, bits):
    for n, nb, ds, dd in shapes():
        plen = pr.packed_block_bytes(n, bits)
        p = pool[n % 777:n % 777 + nb * plen].reshape(nb, plen)
        want = pr.unpack(p, n, bits, elem_dtype(ss))
        got = run_unpack(ctx, p, n, bits, ss, up4(plen) + ds, up4(2 * n * ss) + dd)
        assert np.array_equal(got, want), (n, nb, ds, dd, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("ss,bits", FORMATS, ids=lambda v: str(v))
def test_counts(ctx, ss, bits):
    rng = np.random.default_rng(100 * ss + bits)
    q, dt, info = pr.qmax(bits), elem_dtype(ss), np.iinfo(elem_dtype(ss))
    n, nb = 70001, 5
    stride, dstride = up4(2 * n * ss) + 4, up4(pr.packed_block_bytes(n, bits))
    # all in range: 0, and the pack is the stream itself
    x = rng.integers(-q, q + 1, size=(nb, 2 * n)).astype(dt)
    got, clipped = run_pack(ctx, x, ss, bits, stride, dstride)
    assert clipped == 0 and np.array_equal(got, pr.pack(x, bits)[0])
    assert np.array_equal(run_unpack(ctx, got, n, bits, ss, dstride, stride), x)
    # full-range random elements: the reference's count exactly; the call repeated: the same bytes and the same count
    x = rng.integers(info.min, info.max + 1, size=(nb, 2 * n)).astype(dt)
    want, count = pr.pack(x, bits)
    assert 0 < count < x.size
    for _ in range(3):
        got, clipped = run_pack(ctx, x, ss, bits, stride, dstride)
        assert clipped == count and np.array_equal(got, want)
    # all-extreme streams: every element counted, every field at the clamp
    for v in (info.min, info.max):
        x = np.full((nb, 2 * n), v, dtype=dt)
        got, clipped = run_pack(ctx, x, ss, bits, stride, dstride)
        assert clipped == 2 * n * nb and np.array_equal(got, pr.pack(x, bits)[0])
        assert np.array_equal(run_unpack(ctx, got, n, bits, ss, dstride, stride), np.full((nb, 2 * n), q if v > 0 else -q, dtype=dt))


def test_nothing_to_do_and_optional_outputs(ctx):
    import torch
    buf = torch.full((256,), GUARD, dtype=torch.uint8, device="cuda")
    assert ctx.pack(0, 100, SC08, buf.data_ptr(), 200, PK4, buf.data_ptr() + 128, 100) == (0, 0.0)
    assert ctx.pack(3, 0, SC16, buf.data_ptr(), 0, PK2, buf.data_ptr(), 0) == (0, 0.0)
    assert ctx.unpack(0, 100, PK4, buf.data_ptr(), 100, SC08, buf.data_ptr() + 128, 200) == 0.0
    assert ctx.pack_last_plan()[0] is None
    # clipped and kernel_ms may be NULL
    src = torch.from_numpy(np.arange(64, dtype=np.uint8)).cuda()
    assert gpsiq._pack(ctx._h, 1, 32, SC08, C.c_void_p(src.data_ptr()), 64, PK4, C.c_void_p(buf.data_ptr()), 32, None, None, None) == 0
    assert gpsiq._unpack(ctx._h, 1, 16, PK4, C.c_void_p(buf.data_ptr()), 16, SC08, C.c_void_p(buf.data_ptr() + 64), 32, None, None) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:32], pr.pack(np.arange(64, dtype=np.uint8).view(np.int8), PK4)[0]) and (got[96:] == GUARD).all()
    assert np.array_equal(got[64:96].view(np.int8), pr.unpack(got[:16], 16, PK4))


# ---- a rendered stream ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [PK4, PK2])
def test_round_trip_of_a_rendered_stream(ctx, bits):
    """gpsiq_launch renders 3 blocks at 2.6 Msps, 16 channels, levelled for the format (4 bits: noise at 45 dB-Hz, the level at a third
    of qmax 7; 2 bits: qmax 1 with the level at the clamp): the packer clamps nothing, unpack(pack(x)) is x byte for byte, and
    gpsiq_despread of the unpacked stream gives the integers of the original"""
    import torch
    fs, nchan, nb, nsamp, seg = 2.6e6, 16, 3, 26001, 2560
    desc = synth_blocks(nb, nchan, seed=40 + bits)
    q = gpsiq.quantize_blocks(desc, fs, nsamp)[0]
    qmax = pr.qmax(bits)
    sigma = gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs) if bits == PK4 else 0.0
    stride, plen = up4(2 * nsamp) + 4, pr.packed_block_bytes(nsamp, bits)
    pstride = up4(plen)
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.full((nb * stride,), GUARD, dtype=torch.uint8, device="cuda")
    packed = torch.full((nb * pstride,), GUARD, dtype=torch.uint8, device="cuda")
    back = torch.full((nb * stride,), GUARD, dtype=torch.uint8, device="cuda")
    try:
        if sigma:
            ctx.set_noise(9, sigma, 0)
        ctx.set_level(gpsiq.level_mult(gpsiq.composite_rms(desc["gain"][0], sigma), qmax / 3.0 if bits == PK4 else float(qmax)), qmax)
        ctx.set_descriptors(q)
        ctx.launch(0, nb, nsamp, SC08, raw.data_ptr(), stride, stream=s)
        clipped, _ = ctx.pack(nb, nsamp, SC08, raw.data_ptr(), stride, bits, packed.data_ptr(), pstride, stream=s)
        ctx.unpack(nb, nsamp, bits, packed.data_ptr(), pstride, SC08, back.data_ptr(), stride, stream=s)
        x = raw.cpu().numpy().reshape(nb, stride)
        assert clipped == 0 and np.abs(x[:, :2 * nsamp].view(np.int8)).max() == qmax and (x[:, 2 * nsamp:] == GUARD).all()
        assert np.array_equal(back.cpu().numpy().reshape(nb, stride), x)                   # byte for byte, guards included
        assert np.array_equal(packed.cpu().numpy().reshape(nb, pstride)[:, :plen], pr.pack(x[:, :2 * nsamp].view(np.int8), bits)[0])
        a = ctx.despread(0, nb, nsamp, SC08, raw.data_ptr(), stride, seg, clip=qmax, stream=s)
        b = ctx.despread(0, nb, nsamp, SC08, back.data_ptr(), stride, seg, clip=qmax, stream=s)
        assert a[0].view(np.int64).any() and all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
    finally:
        ctx.noise_off()
        ctx.level_off()


# ---- the packed batch call ------------------------------------------------------------------------------------------------------

BATCH = dict(fs=2.6e6, nblocks=40, nsamp=2600, nchan=16, piece=7)


def batch_descriptors(seed):
    """40 blocks; a satellite change on a piece edge (block 14 with pieces of 7) and one inside a piece (block 10); an unused slot"""
    d = synth_blocks(BATCH["nblocks"], BATCH["nchan"], seed=seed)
    d["prn"][14:, 3] = 29
    d["carr_phase"][14:, 3] = 0.3125
    d["prn"][10:, 5] = 30
    d["carr_phase"][10:, 5] = 0.71875
    d["prn"][:, 9] = 0
    d["prn"][21:, 11] = 0                      # a slot that falls silent on a piece edge
    return d


def settings(c, mode, bits):
    fs = BATCH["fs"]
    sigma = gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs)
    c.set_nco_mode(mode)
    c.set_noise(77, sigma, 5)
    q = pr.qmax(bits)
    c.set_level(gpsiq.level_mult(gpsiq.composite_rms(np.full(8, 0.6), sigma), q / 3.0 if bits == PK4 else 1.0), q)


@pytest.mark.parametrize("mode", [NCO_FIXED, NCO_REFERENCE], ids=["fixed", "reference"])
@pytest.mark.parametrize("bits", [PK4, PK2])
def test_batch_packed_is_the_pack_of_one_batch_call(mode, bits, monkeypatch):
    """six pieces (7 blocks each, the last one 5) against ONE gpsiq_generate_batch over the whole timeline on a second context, then
    a second call that continues the first on both; a host stride of packed + 3 with guard bytes; pageable and page-locked"""
    import torch
    monkeypatch.setenv("GPSIQ_PACK_PIECE_BLOCKS", str(BATCH["piece"]))
    fs, nb, nsamp, nc = BATCH["fs"], BATCH["nblocks"], BATCH["nsamp"], BATCH["nchan"]
    plen = pr.packed_block_bytes(nsamp, bits)
    stride = plen + 3
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        settings(a, mode, bits)
        settings(b, mode, bits)
        d1, d2 = batch_descriptors(500 + bits), batch_descriptors(600 + bits)
        carr_a, carr_b = np.zeros(nc), np.zeros(nc)
        # call 1: pageable destination
        host = np.full(nb * stride + TAIL, GUARD, dtype=np.uint8)
        a.generate_batch_packed(d1, nsamp, fs, bits, host_ptr=host.ctypes.data, block_stride=stride, carr_out=carr_a)
        assert a.pack_last_plan()[3] == 6
        want = b.generate_batch(d1, nsamp, fs, SC08, carr_out=carr_b)
        assert np.abs(want).max() == pr.qmax(bits)
        body = host[:nb * stride].reshape(nb, stride)
        wp, count = pr.pack(want, bits)
        assert count == 0 and np.array_equal(body[:, :plen], wp), np.argwhere(body[:, :plen] != wp)[:4]
        assert (body[:, plen:] == GUARD).all() and (host[nb * stride:] == GUARD).all()
        assert carr_a.tobytes() == carr_b.tobytes()
        # call 2 continues call 1 (the slots that keep their satellite take the phase handed out): page-locked destination
        keep = d2["prn"][0] == d1["prn"][-1]
        d2["carr_phase"][0, keep] = carr_a[keep]
        pinned = torch.full((nb * stride + TAIL,), GUARD, dtype=torch.uint8).pin_memory()
        a.generate_batch_packed(d2, nsamp, fs, bits, host_ptr=pinned.data_ptr(), block_stride=stride, carr_out=carr_a)
        want2 = b.generate_batch(d2, nsamp, fs, SC08, carr_out=carr_b)
        got2 = pinned.numpy()
        assert np.array_equal(got2[:nb * stride].reshape(nb, stride)[:, :plen], pr.pack(want2, bits)[0])
        assert (got2[:nb * stride].reshape(nb, stride)[:, plen:] == GUARD).all() and (got2[nb * stride:] == GUARD).all()
        assert carr_a.tobytes() == carr_b.tobytes() and not np.array_equal(want2, want)
        assert a.noise_state() == b.noise_state()
        # the default piece (one here) and the returned array
        monkeypatch.delenv("GPSIQ_PACK_PIECE_BLOCKS")
        a.set_noise(77, gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs), 5)
        out = a.generate_batch_packed(d1, nsamp, fs, bits)
        assert a.pack_last_plan()[3] == 1 and out.shape == (nb, plen)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("bits", [PK4, PK2])
def test_batch_packed_with_an_odd_nsamp(bits, monkeypatch):
    """2 601 samples per block: the rendered blocks lie 5 202 bytes apart, every other one 2 bytes off a dword, and a PK2 block ends in
    a half-used byte.  Three pieces (5, 5 and 2 blocks) against ONE gpsiq_generate_batch, the host rows back to back and 1 byte apart"""
    monkeypatch.setenv("GPSIQ_PACK_PIECE_BLOCKS", "5")
    fs, nb, nsamp, nc = BATCH["fs"], 12, 2601, BATCH["nchan"]
    plen = pr.packed_block_bytes(nsamp, bits)
    a, b = gpsiq.Context(0), gpsiq.Context(0)
    try:
        settings(a, NCO_FIXED, bits)
        settings(b, NCO_FIXED, bits)
        d = batch_descriptors(700 + bits)[:nb]
        carr_a, carr_b = np.zeros(nc), np.zeros(nc)
        want = b.generate_batch(d, nsamp, fs, SC08, carr_out=carr_b)
        wp, count = pr.pack(want, bits)
        assert count == 0 and np.abs(want).max() == pr.qmax(bits)
        for stride in (plen, plen + 1):
            a.set_noise(77, gpsiq.noise_sigma_for_cn0(45.0, 1.0, fs), 5)
            host = np.full(nb * stride + TAIL, GUARD, dtype=np.uint8)
            a.generate_batch_packed(d, nsamp, fs, bits, host_ptr=host.ctypes.data, block_stride=stride, carr_out=carr_a)
            assert a.pack_last_plan()[3] == 3
            body = host[:nb * stride].reshape(nb, stride)
            assert np.array_equal(body[:, :plen], wp), np.argwhere(body[:, :plen] != wp)[:4]
            assert (body[:, plen:] == GUARD).all() and (host[nb * stride:] == GUARD).all()
            assert carr_a.tobytes() == carr_b.tobytes()
        if bits == PK2:
            assert not (wp[:, -1] >> 4).any()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("bits,fs,flags", [(PK4, 2.6e6, ("--cn0", "45", "--seed", "7", "--level", "2.3")), (PK2, 2600010.0, ("--level", "0.6"))],
                         ids=["4 bit", "2 bit, odd nsamp"])
def test_runahead_pack_flag(tmp_path, monkeypatch, bits, fs, flags):
    """gpsiq_runahead --pack writes the pack of the file the same flags write with --qmax at the format's clamp: block size, stride
    and the size of the write (2 bits at 2 600 010 sps: 260 001 samples per block, the last byte of every block half used)"""
    from test_pipeline import WEEK, horizon_scenario
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-sdr-gps-sim_amd", "host")
    subprocess.run(["make", "-s", "-C", host], check=True)
    monkeypatch.setenv("GPSIQ_PACK_PIECE_BLOCKS", "2")          # two pieces
    nblocks, nchan, ns = 3, 8, int(np.floor(fs / 10.0 + 0.5))
    path, eph, ieph, utc, xyz, sec = horizon_scenario(tmp_path, nblocks, seed=8, sec=270026.0)
    xyz.tofile(str(tmp_path / "xyz.bin"))

    def run(*more):
        out = str(tmp_path / "o.bin")
        r = subprocess.run([os.path.join(host, "gpsiq_runahead"), path, "2", str(WEEK), repr(sec), str(tmp_path / "xyz.bin"),
                            str(nblocks), str(nchan), repr(fs), "1", out, *flags, *more], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.fromfile(out, dtype=np.uint8)
    levelled = run("--qmax", str(pr.qmax(bits))).view(np.int8).reshape(nblocks, 2 * ns)
    assert np.abs(levelled).max() == pr.qmax(bits)
    want, count = pr.pack(levelled, bits)
    got = run("--pack", str(bits))
    assert count == 0 and got.size == nblocks * pr.packed_block_bytes(ns, bits) and np.array_equal(got.reshape(nblocks, -1), want)


def test_errors(ctx):
    import torch
    n = 4096
    buf = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def pack(nblocks=2, nsamp=n, ss=SC08, src=p, sstride=2 * n, bits=PK4, dst=p + 4 * n, dstride=n):
        return ctx.pack(nblocks, nsamp, ss, src, sstride, bits, dst, dstride)

    def unpack(nblocks=2, nsamp=n, bits=PK4, src=p + 4 * n, sstride=n, ss=SC08, dst=p, dstride=2 * n):
        return ctx.unpack(nblocks, nsamp, bits, src, sstride, ss, dst, dstride)

    pack()
    unpack()
    for call in (pack, unpack):
        for kw, word in [(dict(bits=3), "bad bits"), (dict(bits=0), "bad bits"), (dict(bits=8), "bad bits"), (dict(ss=4), "bad sample size"),
                         (dict(sstride=(2 * n if call is pack else n) + 2), "not a multiple of 4"), (dict(dstride=(n if call is pack else 2 * n) + 1), "not a multiple of 4"),
                         (dict(sstride=(2 * n if call is pack else n) - 4), "too small"), (dict(dstride=(n if call is pack else 2 * n) - 4), "too small"),
                         (dict(src=p + 2 + (0 if call is pack else 4 * n)), "not 4-byte aligned"), (dict(dst=p + 1 + (4 * n if call is pack else 0)), "not 4-byte aligned"),
                         (dict(nsamp=-1), "negative size"), (dict(nblocks=-1), "negative size"),
                         (dict(dst=p + 2 * n) if call is pack else dict(dst=p + 3 * n), "overlap"), (dict(dst=p, src=p + 4) if call is pack else dict(src=p), "overlap")]:
            with pytest.raises(gpsiq.GpsiqError) as e:
                call(**kw)
            assert e.value.code == -1 and word in str(e.value), (call.__name__, kw, str(e.value))
    # the batch call: the level off, a clamp outside the format -> GPSIQ_E_STATE; bad bits, a stride below the block -> GPSIQ_E_ARG
    d = synth_blocks(2, 4, seed=3)
    for level, bits, kw, code in [(None, PK4, {}, -5), ((65536, 8), PK4, {}, -5), ((65536, 7), PK2, {}, -5), ((65536, 127), PK2, {}, -5),
                                  ((65536, 7), 3, {}, -1), ((65536, 1), PK2, dict(block_stride=(n + 1) // 2 - 1), -1)]:
        ctx.level_off() if level is None else ctx.set_level(*level)
        try:
            with pytest.raises(gpsiq.GpsiqError) as e:
                ctx.generate_batch_packed(d, kw.pop("nsamp", n), 2.6e6, bits, **kw)
            assert e.value.code == code, (level, bits, str(e.value))
        finally:
            ctx.level_off()
