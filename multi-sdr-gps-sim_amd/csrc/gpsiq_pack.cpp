// gpsiq_pack.cpp -- host side of gpsiq_pack, gpsiq_unpack and gpsiq_generate_batch_packed (include/gpsiq_rows.h, "Packed streams"):
// checks, plan (gpsiq_pack_plan.h, pure and pinned on the CPU), kernel look-up (gpsiq_pack_kernels.hip holds the kernels and the
// table of those that exist), launch, and the batch call's pieces.  libgpsiq_rows.so exports the typed calls and reaches these
// through the plumbing entries "pack", "unpack" and "generate_batch_packed".  Host code: nothing here decides device code, so the
// file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_pack.h"
#include "gpsiq_pack_plan.h"

using namespace gpsiq;

// the words and codes of gpsiq_launch's checks (check_launch, gpsiq_device.cpp), for a source and a destination; src_len / dst_len: the bytes
// of one block on either side
static int check_pack(const gpsiq_ctx *c, int nblocks, int nsamp, int sample_size, int bits, const void *src, size_t src_stride, size_t src_len,
                      const void *dst, size_t dst_stride, size_t dst_len)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (bits != 4 && bits != 2) return fail(GPSIQ_E_ARG, "bad bits %d: 4 or 2", bits);
    if (nsamp < 0 || nblocks < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!src && nblocks && nsamp) return fail(GPSIQ_E_ARG, "null source");
    if (!dst && nblocks && nsamp) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    if (src_stride < src_len || (src_stride & 3)) return fail(GPSIQ_E_ARG, "source block stride %zu too small or not a multiple of 4", src_stride);
    if (dst_stride < dst_len || (dst_stride & 3)) return fail(GPSIQ_E_ARG, "destination block stride %zu too small or not a multiple of 4", dst_stride);
    if (nblocks && nsamp) {
        const uintptr_t s0 = (uintptr_t) src, s1 = s0 + (size_t) (nblocks - 1) * src_stride + src_len;
        const uintptr_t d0 = (uintptr_t) dst, d1 = d0 + (size_t) (nblocks - 1) * dst_stride + dst_len;
        if (s0 < d1 && d0 < s1) return fail(GPSIQ_E_ARG, "source [%p, +%zu) and destination [%p, +%zu) overlap", src, (size_t) (s1 - s0), dst, (size_t) (d1 - d0));
    }
    return GPSIQ_OK;
}

static void note_plan(gpsiq_ctx *c, const PackPlan &p, long pieces)
{
    c->pack.last[0] = p.launch ? (long) p.grid : -1; c->pack.last[1] = (long) p.units; c->pack.last[2] = (long) p.tiles; c->pack.last[3] = pieces;
}

// the packer queued on s: the counter is NOT zeroed here (the batch call adds its pieces up and looks at the sum once, at its end)
static int queue_pack(gpsiq_ctx *c, const PackPlan &p, int nsamp, int sample_size, int bits, const uint8_t *src, size_t src_stride, uint8_t *dst,
                      size_t dst_stride, hipStream_t s)
{
    const PackFn kernel = pack_kernel(sample_size, bits);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no pack kernel for %d-byte samples, %d bits", sample_size, bits);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, src, src_stride, dst, dst_stride, nsamp, p.units, p.tiles, p.total, c->pack.clip.d_count.get());
    HIP_TRY(hipGetLastError());
    return GPSIQ_OK;
}

int gpsiq_pack_impl(gpsiq_ctx_t *c, int nblocks, int nsamp, int sample_size, const void *src, size_t src_stride, int bits, void *dst, size_t dst_stride,
                    void *hip_stream, uint64_t *clipped, float *kernel_ms)
{
    const size_t src_len = block_bytes(nsamp > 0 ? nsamp : 0, sample_size), dst_len = packed_block_bytes(nsamp, bits);
    if (int rc = check_pack(c, nblocks, nsamp, sample_size, bits, src, src_stride, src_len, dst, dst_stride, dst_len)) return rc;
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    const PackPlan p = plan_pack(nblocks, nsamp, sample_size, bits);
    note_plan(c, p, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no byte: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    PackSet &k = c->pack;
    if (int rc = k.reserve()) return rc;
    return counted_call(k.clip, s, [&] {
        return queue_pack(c, p, nsamp, sample_size, bits, static_cast<const uint8_t *>(src), src_stride, static_cast<uint8_t *>(dst), dst_stride, s);
    }, clipped, kernel_ms);
}

int gpsiq_unpack_impl(gpsiq_ctx_t *c, int nblocks, int nsamp, int bits, const void *src, size_t src_stride, int sample_size, void *dst, size_t dst_stride,
                      void *hip_stream, float *kernel_ms)
{
    const size_t dst_len = block_bytes(nsamp > 0 ? nsamp : 0, sample_size), src_len = packed_block_bytes(nsamp, bits);
    if (int rc = check_pack(c, nblocks, nsamp, sample_size, bits, src, src_stride, src_len, dst, dst_stride, dst_len)) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    const PackPlan p = plan_unpack(nblocks, nsamp, bits, sample_size);
    note_plan(c, p, 0);
    if (!p.launch) return GPSIQ_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    ClipCount &k = c->pack.clip;                                      // (the two events of it: unpacking clamps nothing)
    if (int rc = k.reserve()) return rc;
    const UnpackFn kernel = unpack_kernel(bits, sample_size);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no unpack kernel for %d bits, %d-byte samples", bits, sample_size);
    HIP_TRY(hipEventRecord(k.t0.get(), s));
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, static_cast<const uint8_t *>(src), src_stride, static_cast<uint8_t *>(dst), dst_stride,
                       nsamp, p.units, p.tiles, p.total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(k.t1.get(), s));
    HIP_TRY(hipStreamSynchronize(s));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.t0.get(), k.t1.get()));
    return GPSIQ_OK;
}

// The pieces of gpsiq_stage_batch.h with the packer as the stage: the rendered blocks of a piece are packed into d_out[pair], rows of
// `pstride` bytes.  gpsiq_generate_batch lays the rendered blocks back to back.  With an even nsamp every one of them is a packer's
// source where it lies.  With an odd nsamp every other block starts 2 bytes off a dword: the blocks are rendered behind the rows the
// packer reads, lead = `raw` bytes into the same buffer, and a device copy on the stage stream moves them to rows of `sstride` bytes
// first -- nothing reads [0, raw) of the ring, whatever an earlier call left there, before that copy has written it.
int gpsiq_generate_batch_packed_impl(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int bits, void *dst,
                                     size_t dst_block_stride, double *carr_phase_out)
{
    if (!c || (!ch && nblocks) || (!dst && nblocks && nsamp)) return fail(GPSIQ_E_ARG, "null argument");
    if (bits != 4 && bits != 2) return fail(GPSIQ_E_ARG, "bad bits %d: 4 or 2", bits);
    if (int rc = check_batch_shape(nblocks, nchan, nsamp, fs)) return rc;
    const size_t plen = packed_block_bytes(nsamp, bits), blk_bytes = block_bytes(nsamp, GPSIQ_SC08);
    if (dst_block_stride < plen) return fail(GPSIQ_E_ARG, "block stride %zu too small", dst_block_stride);
    const int qmax = bits == 4 ? 7 : 1;
    if (!c->level.mult || c->level.qmax > qmax)
        return fail(GPSIQ_E_STATE, "packed output at %d bits needs the output level on with qmax <= %d (gpsiq_set_level)", bits, qmax);
    if (nblocks == 0) return GPSIQ_OK;                                // an empty batch leaves the carried phases alone
    const char *env = std::getenv("GPSIQ_PACK_PIECE_BLOCKS");
    const int piece = pack_piece_blocks(nblocks, blk_bytes, env ? std::atol(env) : 0);
    const size_t pstride = (plen + 3) & ~(size_t) 3;
    const size_t sstride = (blk_bytes + 3) & ~(size_t) 3, raw = sstride != blk_bytes ? sstride * (size_t) piece : 0;
    if (int rc = gpsiq_stage_batch_begin(c, "gpsiq_generate_batch_packed", ch, raw + blk_bytes * (size_t) piece + 4, pstride * (size_t) piece + 4)) return rc;      // (+4: never a request of no bytes)
    PackSet &k = c->pack;
    if (int rc = k.reserve()) return rc;
    const StageBatch st = {"packed batch", GPSIQ_SC08, raw, 0, piece, k.clip.d_count.get(), k.clip.h_count.get()};
    note_plan(c, plan_pack(piece, nsamp, GPSIQ_SC08, bits), (nblocks + piece - 1) / piece);
    const hipStream_t ss = c->ring.stage_stream.get();
    const int rc0 = [&]() -> int { HIP_TRY(hipMemsetAsync(k.clip.d_count.get(), 0, sizeof(unsigned long long), ss)); return GPSIQ_OK; }();
    double carr[GPSIQ_MAX_CHAN] = {};
    uint64_t clamped = 0;
    const int rc = gpsiq_stage_batch_run(c, st, rc0, ch, nblocks, nchan, nsamp, fs, [&](const Piece &pc, PieceCopy *cp) -> int {
        uint8_t *rows = c->ring.d_render[pc.pair].get(), *out = c->ring.d_out[pc.pair].get();
        const hipError_t e = raw ? hipMemcpy2DAsync(rows, sstride, pc.span, blk_bytes, blk_bytes, (size_t) pc.nb, hipMemcpyDeviceToDevice, ss) : hipSuccess;
        if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "packed batch piece: %s", hipGetErrorString(e));
        if (int rq = queue_pack(c, plan_pack(pc.nb, nsamp, GPSIQ_SC08, bits), nsamp, GPSIQ_SC08, bits, rows, sstride, out, pstride, ss)) return rq;
        *cp = {out, pstride, plen, (size_t) pc.nb, static_cast<uint8_t *>(dst) + (size_t) pc.b0 * dst_block_stride, dst_block_stride};
        return GPSIQ_OK;
    }, carr, &clamped);
    if (rc != GPSIQ_OK) return rc;
    // the level stage held every element inside the format (checked above): a packer that had to clamp says the stream is not that one
    if (clamped) return fail(GPSIQ_E_DEVICE, "packed batch: the packer clamped %llu elements of a stream levelled to qmax %d", (unsigned long long) clamped, c->level.qmax);
    if (carr_phase_out) std::memcpy(carr_phase_out, carr, sizeof(double) * (size_t) nchan);
    return GPSIQ_OK;
}

extern "C" int gpsiq_pack_last_plan(const gpsiq_ctx_t *c, long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->pack.last[i];
    return GPSIQ_OK;
}
