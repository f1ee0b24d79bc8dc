// gpsiq_array.cpp -- host side of gpsiq_array_cov and gpsiq_array_combine (include/gpsiq_rows.h, "Array"): checks, plan
// (gpsiq_array_plan.h, pure and pinned on the CPU), zeroing of the device scratch, kernel look-up (gpsiq_array_kernels.hip holds the
// kernels and the table of those that exist), launch, copy-back, and the scratch turned into the covariance.  libgpsiq_rows.so exports
// the typed calls and reaches these through the plumbing entries "array_cov" and "array_combine".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_array.h"
#include "gpsiq_array_plan.h"
#include "gpsiq_filter_geometry.h"

using namespace gpsiq;

static_assert(sizeof(gpsiq_ctap_t) == 4, "gpsiq_ctap_t is two int16");
static_assert(kArrMaxShift == kFiltMaxShift && kArrWeightSum == kFiltTapSum, "the combiner's shift range and bound are the complex filter's");

namespace {

static_assert(kArrAuto == 0 && kArrForceGeneric == 1 && kArrForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

// nelem streams of nsamp samples: the array itself, and every pointer where there is something to read, 4-byte aligned
int check_sources(int nelem, const void *const *src, int nsamp, int sample_size, ArraySources *out)
{
    if (nelem < 1 || nelem > kArrMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kArrMaxElem);
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!src) return fail(GPSIQ_E_ARG, "null array of sources");
    for (int e = 0; e < kArrMaxElem; ++e) out->p[e] = nullptr;
    for (int e = 0; e < nelem; ++e) {
        if (!src[e] && nsamp) return fail(GPSIQ_E_ARG, "null source %d", e);
        if ((uintptr_t) src[e] & 3) return fail(GPSIQ_E_ARG, "source %d %p not 4-byte aligned", e, src[e]);
        out->p[e] = static_cast<const uint8_t *>(src[e]);
    }
    return GPSIQ_OK;
}

void note_plan(gpsiq_ctx *c, long kernel, long grid, long run, long nelem)
{
    c->array.last[0] = kernel; c->array.last[1] = grid; c->array.last[2] = run; c->array.last[3] = nelem;
}

}  // namespace

int gpsiq_array_cov_impl(gpsiq_ctx_t *c, int nelem, const void *const *src, int nsamp, int sample_size, void *hip_stream, int64_t *cov, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    ArraySources srcs;
    if (int rc = check_sources(nelem, src, nsamp, sample_size, &srcs)) return rc;
    if (!cov) return fail(GPSIQ_E_ARG, "null result");
    if (kernel_ms) *kernel_ms = 0.0f;
    std::memset(cov, 0, sizeof(int64_t) * 2 * (size_t) nelem * (size_t) nelem);
    const ArrayCovPlan p = plan_array_cov(nelem, nsamp, sample_size, forced_kernel("GPSIQ_ARRAY_KERNEL", "mfma"));
    note_plan(c, -1, 0, 0, nelem);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: the zeros stand
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    ArraySet &k = c->array;
    if (int rc = k.reserve()) return rc;
    HIP_TRY(hipMemsetAsync(k.d_gram.get(), 0, sizeof(unsigned long long) * kArrGramWords, s));   // the workgroups add into it: zeroed per call
    HIP_TRY(hipEventRecord(k.clip.t0.get(), s));
    if (p.kernel == kArrMfma) {
        const ArrayCovMfmaFn kernel = array_cov_mfma_kernel(sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no matrix covariance kernel for %d-byte samples", sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, nelem, nsamp, p.steps, p.run, k.d_gram.get());
    } else {
        const ArrayCovFn kernel = array_cov_generic_kernel(sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no covariance kernel for %d-byte samples", sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, nelem, nsamp, p.runs, k.d_gram.get());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(k.clip.t1.get(), s));
    HIP_TRY(hipMemcpyAsync(k.h_gram.get(), k.d_gram.get(), sizeof(unsigned long long) * kArrGramWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    array_scratch_to_cov(p.kernel, reinterpret_cast<const int64_t *>(k.h_gram.get()), nelem, cov);
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.clip.t0.get(), k.clip.t1.get()));
    note_plan(c, p.kernel, (long) p.grid, (long) p.run, nelem);
    return GPSIQ_OK;
}

int gpsiq_array_combine_impl(gpsiq_ctx_t *c, int nelem, const void *const *src, int nsamp, int sample_size, const gpsiq_ctap_t *w, int shift,
                             int out_sample_size, void *dst, void *hip_stream, uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    ArraySources srcs;
    if (int rc = check_sources(nelem, src, nsamp, sample_size, &srcs)) return rc;
    if (shift < 0 || shift > kArrMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kArrMaxShift);
    if (!w) return fail(GPSIQ_E_ARG, "null weights");
    const int16_t *re_im = &w[0].re;                                  // [nelem][2]: the struct is two int16 and no more
    const long mag = array_weight_sum(re_im, nelem);
    if (mag > kArrWeightSum) return fail(GPSIQ_E_RANGE, "sum |re| + |im| %ld above %ld: the accumulator would not hold the sum", mag, kArrWeightSum);
    if (!dst && nsamp) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    const size_t src_len = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, dst_len = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    for (int e = 0; e < nelem; ++e)
        if (overlap(dst, dst_len, src[e], src_len))
            return fail(GPSIQ_E_ARG, "source %d [%p, +%zu) and destination [%p, +%zu) overlap", e, src[e], src_len, dst, dst_len);
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    const ArrayCombinePlan p = plan_array_combine(nsamp, out_sample_size, (unsigned) ((uintptr_t) dst & 15));
    note_plan(c, -1, 0, 0, nelem);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    ArraySet &k = c->array;
    if (int rc = k.reserve()) return rc;
    ArrayWeights wt;
    for (int e = 0; e < kArrMaxElem; ++e) wt.w[e] = e < nelem ? ((uint32_t) (uint16_t) w[e].re | ((uint32_t) (uint16_t) w[e].im << 16)) : 0u;
    const ArrayCombineFn kernel = array_combine_kernel(sample_size, out_sample_size);
    if (!kernel) return fail(GPSIQ_E_DEVICE, "no combiner kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
    note_plan(c, kArrCombine, (long) p.grid, (long) array_slot_samples(out_sample_size), nelem);
    return counted_call(k.clip, s, [&] {
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, wt, nelem, nsamp, shift, static_cast<uint8_t *>(dst), p.lead, p.slots,
                           k.clip.d_count.get());
        HIP_TRY(hipGetLastError());
        return (int) GPSIQ_OK;
    }, clipped, kernel_ms);
}

extern "C" int gpsiq_array_last_plan(const gpsiq_ctx_t *c, long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->array.last[i];
    return GPSIQ_OK;
}
