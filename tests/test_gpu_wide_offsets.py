"""Offsets past 2^31 and 2^32 on the MI355X: the `size_t` strides of include/gpsiq.h and include/gpsiq_rows.h and "every size is 64-bit
arithmetic" on the device side, where each kernel has its own `dst + (size_t) blk * block_stride`, `src + blk * src_stride`, `m0 + n`
line.  Block layouts put five blocks 2^30 + 4 bytes apart: block 2 starts at 2^31 + 8 and block 4 at 2^32 + 16 from the call's base
pointer, and an offset cut to 32 bits would land inside block 0.  The searches and the follower work on one span whose last samples
lie 4.8e9 bytes (int16) and 2^31 - 1 elements (int8) in.  Buffers are 0x7f wherever no block lies; only the block regions come back
to the host, the gaps and the tail are compared on the device.  The time of this module is allocation and fills, not kernels.
Run with -m gpu."""
import numpy as np
import pytest

import _acquire_plan as ap
import _contract_cases as cc
import _despread_ref as dr
import _oracle
import _pack_ref as pr
import _plan_query as pq
import _stage_cases as sc
import gpsiq
from gpsiq.abi import NCO_FIXED, NCO_REFERENCE, PATCH_DTYPE, SC08, SC16, elem_dtype
from gpsiq.scenario import synth_blocks
from test_gpu_parity import VARIANTS

pytestmark = pytest.mark.gpu

GUARD, W, NB = cc.GUARD, cc.WIDE_STRIDE, cc.WIDE_BLOCKS
NSAMP = 4999
MAX_BLOCK = 4 * NSAMP                               # the longest block of the layouts: 4999 int16 samples
SPAN_BYTES = 4 * cc.WIDE_SEARCHES[0].nsamp + 64     # the int16 span and 64 bytes behind it; the int8 span (2^32 - 2 bytes) fits too
NEED = SPAN_BYTES + cc.wide_bytes(MAX_BLOCK) + (3 << 30)


@pytest.fixture(scope="module")
def wide():
    """(first, second): `first` holds the spans and, in its first wide_bytes(MAX_BLOCK) bytes, a block layout; `second` is the other
    block layout of pack and unpack.  Every byte 0x7f; every test puts back what it wrote."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU path in libgpsiq"
    free, total = torch.cuda.mem_get_info()
    assert free >= NEED, "the wide-offset tests need %.1f GiB of free device memory, %.1f of %.1f GiB are free" % (NEED / 2 ** 30, free / 2 ** 30, total / 2 ** 30)
    first = torch.full((SPAN_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
    second = torch.full((cc.wide_bytes(MAX_BLOCK),), GUARD, dtype=torch.uint8, device="cuda")
    yield first, second
    del first, second
    torch.cuda.empty_cache()


@pytest.fixture()
def layout(wide):
    """the two block layouts, 0x7f again behind the test"""
    a, b = wide[0][:cc.wide_bytes(MAX_BLOCK)], wide[1]
    yield a, b
    for buf in (a, b):
        for k in range(NB):
            buf[k * W:k * W + MAX_BLOCK].fill_(GUARD)


@pytest.fixture(scope="module")
def ctx():
    c = gpsiq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    return _oracle.load_oracle()


def put_blocks(buf, blocks):
    """blocks: [NB][len] elements or bytes -> block k at byte k * W"""
    import torch
    raw = np.ascontiguousarray(blocks).view(np.uint8).reshape(len(blocks), -1)
    for k in range(len(raw)):
        buf[k * W:k * W + raw.shape[1]] = torch.from_numpy(raw[k].copy()).cuda()


def get_blocks(buf, block_bytes, dtype=np.uint8, nblocks=NB):
    """the block regions alone -> [nblocks][block_bytes / itemsize]"""
    return np.stack([buf[k * W:k * W + block_bytes].cpu().numpy() for k in range(nblocks)]).view(dtype)


def assert_guards(buf, block_bytes, nblocks=NB):
    """every byte that belongs to no block is 0x7f: the gaps one by one, then the tail, on the device"""
    for k in range(nblocks):
        lo, hi = k * W + block_bytes, (k + 1) * W if k + 1 < nblocks else buf.numel()
        assert bool((buf[lo:hi] == GUARD).all()), "bytes behind block %d changed (between %d and %d)" % (k, lo, hi)


def differing(got, want):
    return [(b, int(np.flatnonzero(got[b] != want[b])[0])) for b in range(len(want)) if not np.array_equal(got[b], want[b])]


# ---- gpsiq_launch ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ss", [SC08, SC16], ids=["int8", "int16"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_launch_every_variant(ctx, orc, layout, variant, ss):
    q, _ = gpsiq.quantize_blocks(synth_blocks(NB, 7, seed=310 + ss), 2.6e6, NSAMP)
    ctx.set_nco_mode(NCO_FIXED)
    ctx.set_descriptors(q)
    ctx.launch(0, NB, NSAMP, ss, layout[0].data_ptr(), W, variant=gpsiq.variants()[variant])
    ctx.synchronize()
    got = get_blocks(layout[0], 2 * NSAMP * ss, elem_dtype(ss))
    want = np.stack([orc.block_fixed(q[b], NSAMP, ss) for b in range(NB)])
    assert not differing(got, want), differing(got, want)
    assert_guards(layout[0], 2 * NSAMP * ss)


@pytest.mark.parametrize("stage", sc.STAGES)
def test_launch_noise_and_level_families(ctx, orc, layout, stage):
    """one case of tests/_stage_cases.py per stage (noise, level over noise, level alone), five blocks of 4999 samples"""
    from test_gpu_stage_matrix import Resident, apply
    c = [k for k in sc.CASES if k.stage == stage and k.rate == "row" and k.env == "" and k.ss == (SC08 if stage == sc.LEVEL else SC16)][0]
    c = c._replace(nsamp=NSAMP, nblocks=NB)
    st = sc.settings(c)
    res = Resident(orc, sc.descriptors(c), NSAMP)
    plan = pq.query(c.variant, c.ss, NSAMP, NB, res.cls, None if st.sigma is None else sc.max_z(st.sigma), st.level is not None)
    assert (plan.kernel, plan.stage) == (sc.kernel_name(c), sc.stage_family(c)), plan
    try:
        apply(ctx, st)
        ctx.set_descriptors(res.q)
        ctx.launch(0, NB, NSAMP, c.ss, layout[0].data_ptr(), W, variant=gpsiq.variants()[c.variant])
        ctx.synchronize()
        got, want = get_blocks(layout[0], 2 * NSAMP * c.ss, elem_dtype(c.ss)), res.want(c.ss, st, 0, NB)
        assert not differing(got, want), differing(got, want)
        assert_guards(layout[0], 2 * NSAMP * c.ss)
    finally:
        ctx.noise_off()
        ctx.level_off()


def test_launch_with_a_patch_in_block_four(orc, layout):
    """GPSIQ_NCO_REFERENCE: the patch kernel has its own offset line.  Patches made by hand in blocks 0, 2 and 4 (the last sample of the
    last block among them), held to tests/_oracle.py's stand-in for the fix-up"""
    q, _ = gpsiq.quantize_blocks(synth_blocks(NB, 5, seed=77), 2.6e6, NSAMP)
    patches = np.array([(0, 17, 1, 1, 300), (2, NSAMP - 1, 0, 0, 5), (4, 2500, 2, 1, 129), (4, NSAMP - 1, 4, 0, 511)], dtype=PATCH_DTYPE)
    plain = np.stack([orc.block_fixed(q[b], NSAMP, SC16) for b in range(NB)])
    want = plain.copy()
    for b in range(NB):
        _oracle.apply_patches(orc, q[b], want[b], patches[patches["block"] == b], SC16)
    assert [b for b, _ in differing(want, plain)] == [0, 2, 4] and (want[4, 2 * 2500:2 * 2501] != plain[4, 2 * 2500:2 * 2501]).any()
    rctx = gpsiq.Context(0)
    try:
        rctx.set_nco_mode(NCO_REFERENCE)
        rctx.set_descriptors(q)
        rctx.set_patches(patches)
        rctx.launch(0, NB, NSAMP, SC16, layout[0].data_ptr(), W)
        rctx.synchronize()
        got = get_blocks(layout[0], 4 * NSAMP, np.int16)
        assert not differing(got, want), differing(got, want)
        assert_guards(layout[0], 4 * NSAMP)
    finally:
        rctx.close()


# ---- gpsiq_despread -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["rows", "generic"])
def test_despread(ctx, orc, layout, kernel, monkeypatch):
    """the source five blocks W apart, through the rows kernel and the generic one; then blocks 2..4 alone from a base at block 2"""
    if kernel == "generic":
        monkeypatch.setenv("GPSIQ_DESPREAD_KERNEL", "generic")
    ss, seg = (SC16, 2560) if kernel == "rows" else (SC08, 1280)
    q, _ = gpsiq.quantize_blocks(synth_blocks(NB, 7, seed=501), 2.6e6, NSAMP)
    info = np.iinfo(elem_dtype(ss))
    stream = np.random.default_rng(502).integers(info.min, info.max + 1, size=(NB, 2 * NSAMP)).astype(elem_dtype(ss))
    put_blocks(layout[0], stream)
    ctx.set_nco_mode(NCO_FIXED)
    ctx.set_descriptors(q)
    clip = cc.DESPREAD_CLIP[ss]
    for block0, nb in ((0, NB), (2, 3)):
        sums, prn, st, _ = ctx.despread(block0, nb, NSAMP, ss, layout[0].data_ptr() + block0 * W, W, seg, clip=clip)
        assert ctx.despread_last_plan()[0] == kernel
        ref_sums, ref_prn = dr.despread(orc, q[block0:block0 + nb], stream[block0:block0 + nb], NSAMP, seg)
        assert np.array_equal(prn, ref_prn) and np.array_equal(sums, ref_sums), np.argwhere(sums != ref_sums)[:5]
        assert np.array_equal(st, dr.stats(stream[block0:block0 + nb], NSAMP, clip))


# ---- gpsiq_pack, gpsiq_unpack ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsamp", [513, NSAMP])
@pytest.mark.parametrize("ss,bits", cc.PACK_FORMATS, ids=lambda v: str(v))
def test_pack_and_unpack(ctx, layout, ss, bits, nsamp):
    """both strides W: the packer from the first layout into the second, the unpacker back into the first"""
    src, dst = layout
    x = np.random.default_rng(600 + 10 * ss + bits + nsamp).integers(0, 256, size=(NB, 2 * nsamp * ss), dtype=np.uint8).view(elem_dtype(ss))
    want, count = pr.pack(x, bits)
    put_blocks(src, x)
    clipped, _ = ctx.pack(NB, nsamp, ss, src.data_ptr(), W, bits, dst.data_ptr(), W)
    got = get_blocks(dst, want.shape[1])
    assert not differing(got, want), differing(got, want)
    assert clipped == count and 0 < count
    assert_guards(dst, want.shape[1])
    for k in range(NB):
        src[k * W:k * W + MAX_BLOCK].fill_(GUARD)
    ctx.unpack(NB, nsamp, bits, dst.data_ptr(), W, ss, src.data_ptr(), W)
    back = get_blocks(src, 2 * nsamp * ss, elem_dtype(ss))
    assert not differing(back, pr.unpack(want, nsamp, bits, elem_dtype(ss)))
    assert_guards(src, 2 * nsamp * ss)


# ---- gpsiq_acquire, gpsiq_follow: one span ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [w.name for w in cc.WIDE_SEARCHES])
def test_acquire_one_span(ctx, wide, name, monkeypatch):
    """two dwells, the second ending on the span's last sample; only the two dwell windows hold elements, the rest of the span and what
    lies behind it is 0x7f.  The digit planes of the matrix path would exceed its scratch cap: the generic kernel, whatever is asked"""
    import torch
    from test_gpu_acquire import same
    w, wins, first, ref = cc.wide_search_reference(name)
    monkeypatch.setenv("GPSIQ_ACQUIRE_KERNEL", "mfma")
    assert ap.query(w.nsamp, w.ss, len(w.prns), w.ndopp, w.nshift, w.ncoh, w.nnoncoh, w.hop, "mfma").kernel == "generic"
    buf = wide[0]
    assert 2 * w.ss * w.nsamp + 2 <= buf.numel()
    try:
        for x, m0 in zip(wins, first):
            buf[2 * w.ss * m0:2 * w.ss * m0 + x.nbytes] = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        got = ctx.acquire(w.nsamp, w.ss, buf.data_ptr(), w.prns, *cc.WIDE_STEPS, w.ndopp, w.nshift, w.ncoh, w.nnoncoh, w.hop, corr=True)
        assert ctx.acquire_last_plan()[0] == "generic"
        same(got, ref)
    finally:
        for x, m0 in zip(wins, first):
            buf[2 * w.ss * m0:2 * w.ss * m0 + x.nbytes].fill_(GUARD)


def test_follow_to_the_end_of_the_span(ctx, wide):
    """two satellites that start some 2800 samples before the end of a span of 1.2e9 int16 samples and run to it, one of them ending
    on the span's last sample: the restatement on the tail, `sample` rebased"""
    import torch
    from test_gpu_follow import same
    nsamp, base, tail, cfg, states, ref = cc.wide_follow_reference()
    buf = wide[0]
    assert 4 * nsamp <= buf.numel()
    try:
        buf[4 * base:4 * base + tail.nbytes] = torch.from_numpy(tail.view(np.uint8).copy()).cuda()
        got = ctx.follow(nsamp, SC16, buf.data_ptr(), cfg, states, cc.WIDE_FOLLOW_MAX_EPOCHS)
        same(got, ref)
        assert [int(s) for s in got[2]["status"]] == [1, 1] and int(got[2][0]["sample"]) == nsamp
    finally:
        buf[4 * base:4 * base + tail.nbytes].fill_(GUARD)
