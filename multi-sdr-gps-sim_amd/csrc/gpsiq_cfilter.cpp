// gpsiq_cfilter.cpp -- host side of gpsiq_cfilter (include/gpsiq_rows.h, "Complex filter and notch"): checks, plan (gpsiq_cfilter_plan.h,
// pure and pinned on the CPU), the taps and the matrix kernels' digit planes on their way to the device, kernel look-up
// (gpsiq_cfilter_kernels.hip holds the stage's kernels; an int8 input on the matrix path takes filter_mfma of gpsiq_filter_kernels.hip
// with the complex planes), launch and count.  libgpsiq_rows.so exports the typed call and reaches this through the plumbing entry
// "cfilter".  Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_cfilter.h"
#include "gpsiq_cfilter_plan.h"

using namespace gpsiq;

static_assert(sizeof(gpsiq_ctap_t) == 4, "gpsiq_ctap_t is two int16");

namespace {

static_assert(kCfiltAuto == 0 && kCfiltForceGeneric == 1 && kCfiltForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

void note_plan(gpsiq_ctx *c, const FilterPlan &p)
{
    c->cfilt.last[0] = p.launch ? (long) p.kernel : -1; c->cfilt.last[1] = (long) p.grid; c->cfilt.last[2] = (long) p.run; c->cfilt.last[3] = (long) p.steps;
}

// The coefficients of a call, page-locked, then queued for the device on s: the taps as dwords (re low, im high), and behind them the
// two digit planes of the matrix kernels (cfilter_build_planes).  Nothing queued earlier still reads h_coef: every call ends
// synchronised.
int stage_coefficients(gpsiq_ctx *c, const int16_t *re_im, int ntaps, int decim, const FilterPlan &p, hipStream_t s)
{
    FirSet &k = c->cfilt;
    std::memcpy(k.h_coef.get(), re_im, 4 * (size_t) ntaps);
    size_t bytes = FirSet::kTapBytes;
    if (p.kernel != kCfiltGeneric) {
        cfilter_build_planes(re_im, ntaps, decim, p.steps, reinterpret_cast<int8_t *>(k.h_coef.get() + FirSet::kTapBytes));
        bytes += (size_t) filter_mfma_plane_bytes(p.steps);
    }
    HIP_TRY(hipMemcpyAsync(k.d_coef.get(), k.h_coef.get(), bytes, hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

// the filter queued on s behind its coefficients (the counter is counted_call's to zero)
int queue_cfilter(gpsiq_ctx *c, const FilterPlan &p, int nsamp, int sample_size, const uint8_t *src, const uint8_t *head, const int16_t *re_im, int ntaps,
                  int shift, int decim, int phase, int out_sample_size, uint8_t *dst, hipStream_t s)
{
    FirSet &k = c->cfilt;
    const uint8_t *planes = k.d_coef.get() + FirSet::kTapBytes;
    if (p.kernel == kCfiltMfma) {
        const FilterMfmaFn kernel = filter_mfma_kernel(out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no matrix filter kernel for %d-byte outputs", out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, planes, ntaps, shift, decim, phase, dst, p.nout, p.run, p.runs, p.steps,
                           k.clip.d_count.get());
    } else if (p.kernel == kCfiltMfma16) {
        const CfilterMfma16Fn kernel = cfilter_mfma16_kernel(out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no int16 matrix filter kernel for %d-byte outputs", out_sample_size);
        int32_t rc2[2];
        cfilter_row_consts(re_im, ntaps, rc2);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, planes, ntaps, shift, decim, phase, dst, p.nout, p.run, p.runs, p.steps,
                           (int) rc2[0], (int) rc2[1], k.clip.d_count.get());
    } else {
        const CfilterGenericFn kernel = cfilter_generic_kernel(sample_size, out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no complex filter kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, reinterpret_cast<const uint32_t *>(k.d_coef.get()), ntaps, shift,
                           decim, phase, dst, p.nout, p.run, p.runs, k.clip.d_count.get());
    }
    HIP_TRY(hipGetLastError());
    return GPSIQ_OK;
}

}  // namespace

int gpsiq_cfilter_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, const void *head, const gpsiq_ctap_t *taps, int ntaps, int shift,
                       int decim, int phase, int out_sample_size, void *dst, void *hip_stream, int *nout, uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    if (ntaps < 1 || ntaps > kFiltMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kFiltMaxTaps);
    if (decim < 1 || decim > kFiltMaxDecim) return fail(GPSIQ_E_ARG, "decim %d outside 1..%d", decim, kFiltMaxDecim);
    if (shift < 0 || shift > kFiltMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kFiltMaxShift);
    if (!taps) return fail(GPSIQ_E_ARG, "null taps");
    const int16_t *re_im = &taps[0].re;                               // [ntaps][2]: the struct is two int16 and no more
    const CtapStats st = cfilter_tap_stats(re_im, ntaps);
    if (st.mag > kCfiltTapSum) return fail(GPSIQ_E_RANGE, "sum |re| + |im| %ld above %ld: the accumulator would not hold the sum", st.mag, kCfiltTapSum);
    if (phase < 0 || phase >= decim) return fail(GPSIQ_E_ARG, "phase %d outside [0, decim %d)", phase, decim);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    const FilterPlan p = plan_cfilter(nsamp, sample_size, ntaps, decim, phase, st, forced_kernel("GPSIQ_CFILTER_KERNEL", "mfma"));
    if (int rc = check_span(src, nsamp, sample_size, head, ntaps, dst, (uint64_t) p.nout, out_sample_size)) return rc;
    if (nout) *nout = p.nout;
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    note_plan(c, p);
    if (!p.launch) return GPSIQ_OK;                                   // no output: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    FirSet &k = c->cfilt;
    if (int rc = k.reserve()) return rc;
    if (int rc = stage_coefficients(c, re_im, ntaps, decim, p, s)) return rc;
    return counted_call(k.clip, s, [&] {
        return queue_cfilter(c, p, nsamp, sample_size, static_cast<const uint8_t *>(src), static_cast<const uint8_t *>(head), re_im, ntaps, shift, decim, phase,
                             out_sample_size, static_cast<uint8_t *>(dst), s);
    }, clipped, kernel_ms);
}

extern "C" int gpsiq_cfilter_last_plan(const gpsiq_ctx_t *c, long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->cfilt.last[i];
    return GPSIQ_OK;
}
