// gpsiq_stap.cpp -- host side of gpsiq_stap_cov and gpsiq_stap_combine (include/gpsiq_rows.h, "Space-time array"): checks, plan
// (gpsiq_stap_plan.h, pure and pinned on the CPU), zeroing of the device scratch, kernel look-up (gpsiq_stap_kernels.hip holds the
// kernels and the table of those that exist), launch, copy-back, and the scratch turned into the covariance.  libgpsiq_rows.so exports
// the typed calls and reaches these through the plumbing entries "stap_cov" and "stap_combine".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_stap.h"
#include "gpsiq_stap_plan.h"
#include "gpsiq_filter_geometry.h"

using namespace gpsiq;

static_assert(sizeof(gpsiq_ctap_t) == 4, "gpsiq_ctap_t is two int16");
static_assert(kStapMaxShift == kFiltMaxShift && kStapWeightSum == kFiltTapSum, "the combiner's shift range and bound are the complex filter's");
static_assert(kStapMaxElem * kStapMaxTaps >= kStapMaxRows && kStapMaxGroups == 4, "the largest shapes fill the Gram matrix");

namespace {

static_assert(kStapAuto == 0 && kStapForceGeneric == 1 && kStapForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

// nelem streams of nsamp samples with ntaps - 1 samples of head each: the sizes, the arrays themselves, and every pointer where there
// is something to read, 4-byte aligned
int check_sources(int nelem, const void *const *src, const void *const *head, int nsamp, int sample_size, int ntaps, StapSources *out)
{
    if (nelem < 1 || nelem > kStapMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kStapMaxElem);
    if (ntaps < 1 || ntaps > kStapMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kStapMaxTaps);
    if (nelem * ntaps > kStapMaxRows) return fail(GPSIQ_E_ARG, "nelem %d * ntaps %d above %d rows", nelem, ntaps, kStapMaxRows);
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!src) return fail(GPSIQ_E_ARG, "null array of sources");
    for (int e = 0; e < kStapMaxElem; ++e) { out->p[e] = nullptr; out->head[e] = nullptr; }
    for (int e = 0; e < nelem; ++e) {
        if (!src[e] && nsamp) return fail(GPSIQ_E_ARG, "null source %d", e);
        if ((uintptr_t) src[e] & 3) return fail(GPSIQ_E_ARG, "source %d %p not 4-byte aligned", e, src[e]);
        out->p[e] = static_cast<const uint8_t *>(src[e]);
        const void *h = head && ntaps > 1 ? head[e] : nullptr;        // (one tap reads nothing before the span)
        if ((uintptr_t) h & 3) return fail(GPSIQ_E_ARG, "head %d %p not 4-byte aligned", e, h);
        out->head[e] = static_cast<const uint8_t *>(h);
    }
    return GPSIQ_OK;
}

void note_plan(gpsiq_ctx *c, long kernel, long grid, long run, long nelem, long ntaps)
{
    c->stap.last[0] = kernel; c->stap.last[1] = grid; c->stap.last[2] = run; c->stap.last[3] = nelem; c->stap.last[4] = ntaps;
}

}  // namespace

int gpsiq_stap_cov_impl(gpsiq_ctx_t *c, int nelem, const void *const *src, const void *const *head, int nsamp, int sample_size, int ntaps,
                        void *hip_stream, int64_t *cov, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    StapSources srcs;
    if (int rc = check_sources(nelem, src, head, nsamp, sample_size, ntaps, &srcs)) return rc;
    if (!cov) return fail(GPSIQ_E_ARG, "null result");
    const int rows = nelem * ntaps;
    if (kernel_ms) *kernel_ms = 0.0f;
    std::memset(cov, 0, sizeof(int64_t) * 2 * (size_t) rows * (size_t) rows);
    const StapCovPlan p = plan_stap_cov(nelem, ntaps, nsamp, sample_size, forced_kernel("GPSIQ_STAP_KERNEL", "mfma"));
    note_plan(c, -1, 0, 0, nelem, ntaps);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: the zeros stand
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    StapSet &k = c->stap;
    if (int rc = k.reserve()) return rc;
    HIP_TRY(hipMemsetAsync(k.d_gram.get(), 0, sizeof(unsigned long long) * kStapGramWords, s));   // the workgroups add into it: zeroed per call
    HIP_TRY(hipEventRecord(k.clip.t0.get(), s));
    if (p.kernel == kStapMfma) {
        const StapCovMfmaFn kernel = stap_cov_mfma_kernel(sample_size, p.groups);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no matrix covariance kernel for %d-byte samples in %d row groups", sample_size, p.groups);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, nelem, ntaps, nsamp, p.steps, p.run, k.d_gram.get());
    } else {
        const StapCovFn kernel = stap_cov_generic_kernel(sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no covariance kernel for %d-byte samples", sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, nelem, ntaps, nsamp, p.runs, k.d_gram.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(k.clip.t1.get(), s));
    HIP_TRY(hipMemcpyAsync(k.h_gram.get(), k.d_gram.get(), sizeof(unsigned long long) * kStapGramWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    stap_scratch_to_cov(p.kernel, reinterpret_cast<const int64_t *>(k.h_gram.get()), rows, cov);
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.clip.t0.get(), k.clip.t1.get()));
    note_plan(c, p.kernel, (long) p.grid, (long) p.run, nelem, ntaps);
    return GPSIQ_OK;
}

int gpsiq_stap_combine_impl(gpsiq_ctx_t *c, int nelem, const void *const *src, const void *const *head, int nsamp, int sample_size,
                            const gpsiq_ctap_t *w, int ntaps, int shift, int out_sample_size, void *dst, void *hip_stream, uint64_t *clipped,
                            float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    StapSources srcs;
    if (int rc = check_sources(nelem, src, head, nsamp, sample_size, ntaps, &srcs)) return rc;
    if (shift < 0 || shift > kStapMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kStapMaxShift);
    if (!w) return fail(GPSIQ_E_ARG, "null weights");
    const int rows = nelem * ntaps;
    const int16_t *re_im = &w[0].re;                                  // [nelem][ntaps][2]: the struct is two int16 and no more
    const long mag = stap_weight_sum(re_im, rows);
    if (mag > kStapWeightSum) return fail(GPSIQ_E_RANGE, "sum |re| + |im| %ld above %ld: the accumulator would not hold the sum", mag, kStapWeightSum);
    if (!dst && nsamp) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    const size_t src_len = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, dst_len = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    const size_t head_len = (size_t) 2 * (size_t) (ntaps - 1) * (size_t) sample_size;
    for (int e = 0; e < nelem; ++e) {
        if (overlap(dst, dst_len, src[e], src_len))
            return fail(GPSIQ_E_ARG, "source %d [%p, +%zu) and destination [%p, +%zu) overlap", e, src[e], src_len, dst, dst_len);
        if (srcs.head[e] && overlap(dst, dst_len, srcs.head[e], head_len))
            return fail(GPSIQ_E_ARG, "head %d [%p, +%zu) and destination [%p, +%zu) overlap", e, (const void *) srcs.head[e], head_len, dst, dst_len);
    }
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    const StapCombinePlan p = plan_stap_combine(nsamp, out_sample_size, (unsigned) ((uintptr_t) dst & 15));
    note_plan(c, -1, 0, 0, nelem, ntaps);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    StapSet &k = c->stap;
    if (int rc = k.reserve()) return rc;
    StapWeights wt;
    for (int r = 0; r < kStapMaxRows; ++r) wt.w[r] = r < rows ? ((uint32_t) (uint16_t) w[r].re | ((uint32_t) (uint16_t) w[r].im << 16)) : 0u;
    const StapCombineFn kernel = stap_combine_kernel(sample_size, out_sample_size);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no combiner kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
    note_plan(c, kStapCombine, (long) p.grid, (long) stap_slot_samples(out_sample_size), nelem, ntaps);
    return counted_call(k.clip, s, [&] {
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, wt, nelem, ntaps, nsamp, shift, static_cast<uint8_t *>(dst), p.lead, p.slots,
                           k.clip.d_count.get());
        HIP_TRY(hipGetLastError());
        return (int) GPSIQ_OK;
    }, clipped, kernel_ms);
}

extern "C" int gpsiq_stap_last_plan(const gpsiq_ctx_t *c, long out[5])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 5; ++i) out[i] = c->stap.last[i];
    return GPSIQ_OK;
}
