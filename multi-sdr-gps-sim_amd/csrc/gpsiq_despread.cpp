// gpsiq_despread.cpp -- host side of gpsiq_despread (include/gpsiq_rows.h, "Despread"): checks, plan (gpsiq_despread_plan.h, pure
// and pinned on the CPU), kernel look-up (gpsiq_despread_kernels.hip holds the kernels and the table of those that exist), zeroing,
// launch, copy-back.  libgpsiq_rows.so exports the typed call and reaches this through the plumbing entry "despread".  Host code:
// nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_despread.h"
#include "gpsiq_despread_plan.h"

using namespace gpsiq;

// the words and codes of gpsiq_launch's checks (check_launch, gpsiq_device.cpp), for a source instead of a destination
static int check_despread(const gpsiq_ctx *c, int block0, int nblocks, int nsamp, int sample_size, const void *src, size_t stride,
                          int seg_len, const void *sums, const void *prn)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0 || nblocks < 0 || block0 < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (seg_len < 64 || (seg_len & 63)) return fail(GPSIQ_E_ARG, "segment length %d: a multiple of 64, at least 64", seg_len);
    if (!c->d_desc || nblocks > c->nblocks || block0 > c->nblocks - nblocks)        // no int overflow in the sum
        return fail(GPSIQ_E_STATE, "blocks [%d,+%d) not resident (have %d)", block0, nblocks, c->nblocks);
    if (!src && nblocks && nsamp) return fail(GPSIQ_E_ARG, "null source");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    if (stride < block_bytes(nsamp, sample_size) || (stride & 3))
        return fail(GPSIQ_E_ARG, "block stride %zu too small or not a multiple of 4", stride);
    if (nblocks && (!prn || (!sums && nsamp))) return fail(GPSIQ_E_ARG, "null output");
    return GPSIQ_OK;
}

int gpsiq_despread_impl(gpsiq_ctx_t *c, int block0, int nblocks, int nsamp, int sample_size, const void *src, size_t block_stride_bytes,
                        void *hip_stream, int seg_len, int clip, gpsiq_despread_sum_t *sums, uint8_t *prn, gpsiq_block_stats_t *stats,
                        float *kernel_ms)
{
    if (int rc = check_despread(c, block0, nblocks, nsamp, sample_size, src, block_stride_bytes, seg_len, sums, prn)) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    const char *force = std::getenv("GPSIQ_DESPREAD_KERNEL");
    const char *target = std::getenv("GPSIQ_DESPREAD_TARGET_WGS");
    const DespreadPlan p = plan_despread(nsamp, nblocks, seg_len, c->cls, force && !std::strcmp(force, "generic"),
                                         target && std::atoi(target) > 0 ? std::atoi(target) : kDespreadTargetWgs);
    c->dsp.last[0] = p.kind == kPlanLaunch ? p.kernel : -1; c->dsp.last[1] = p.slots; c->dsp.last[2] = (int) p.grid; c->dsp.last[3] = p.wave_rows;
    if (p.kind != kPlanLaunch) return GPSIQ_OK;                       // no block: no output to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    DespreadSet &d = c->dsp;
    const size_t nprn = (size_t) nblocks * (size_t) c->nchan, nsums = nprn * (size_t) p.nseg;
    if (int rc = d.reserve(nsums ? nsums : 1, nprn, (size_t) nblocks)) return rc;
    const DespreadFn kernel = despread_kernel(sample_size, p.kernel, p.slots);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no correlator kernel %s for %d slots, %d-byte samples", despread_kernel_name(p.kernel), p.slots, sample_size);

    gpsiq_ctx::DescBuf &cb = c->buf[c->cur];
    if (cb.upload_pending) HIP_TRY(hipStreamWaitEvent(s, cb.uploaded.get(), 0));      // a set staged without waiting
    // the waves add into the sums and the statistics: this call zeroes them itself
    if (nsums) HIP_TRY(hipMemsetAsync(d.d_sums.get(), 0, nsums * sizeof(gpsiq_despread_sum_t), s));
    if (stats) HIP_TRY(hipMemsetAsync(d.d_stats.get(), 0, (size_t) nblocks * sizeof(gpsiq_block_stats_t), s));
    HIP_TRY(hipEventRecord(d.t0.get(), s));
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, c->d_desc, c->nchan, nsamp, static_cast<const uint8_t *>(src), block_stride_bytes,
                       block0, c->d_tab.get(), p.tiles, p.wave_rows, p.seg_rows, p.nseg > 0 ? p.nseg : 1, clip, d.d_sums.get(), d.d_prn.get(),
                       stats ? d.d_stats.get() : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d.t1.get(), s));
    if (int rc = gpsiq_mark_use(cb, s)) return rc;                   // the descriptor set is being read
    if (nsums) HIP_TRY(hipMemcpyAsync(d.h_sums.get(), d.d_sums.get(), nsums * sizeof(gpsiq_despread_sum_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(d.h_prn.get(), d.d_prn.get(), nprn, hipMemcpyDeviceToHost, s));
    if (stats) HIP_TRY(hipMemcpyAsync(d.h_stats.get(), d.d_stats.get(), (size_t) nblocks * sizeof(gpsiq_block_stats_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nsums) std::memcpy(sums, d.h_sums.get(), nsums * sizeof(gpsiq_despread_sum_t));
    std::memcpy(prn, d.h_prn.get(), nprn);
    if (stats) std::memcpy(stats, d.h_stats.get(), (size_t) nblocks * sizeof(gpsiq_block_stats_t));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, d.t0.get(), d.t1.get()));
    return GPSIQ_OK;
}

extern "C" int gpsiq_despread_last_plan(const gpsiq_ctx_t *c, int out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->dsp.last[i];
    return GPSIQ_OK;
}
