// gpsiq_stap_beams.cpp -- host side of gpsiq_stap_beams (include/gpsiq_rows.h, "Space-time array"): checks, the overlap rules over the
// sources, the heads and every destination, plan (gpsiq_stap_beams_plan.h, pure and pinned on the CPU), the coefficients on their way
// to the device, kernel look-up (gpsiq_stap_beams_kernels.hip holds the kernels and the table of those that exist), launch, and the
// counts' way back.  libgpsiq_rows.so exports the typed call and reaches this through the plumbing entry "stap_beams".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_stap_beams.h"
#include "gpsiq_stap_beams_plan.h"

using namespace gpsiq;

static_assert(kBeamsAuto == 0 && kBeamsForceGeneric == 1 && kBeamsForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

namespace {

void note_plan(gpsiq_ctx *c, long kernel, long grid, long run, long nelem, long ntaps, long nbeams, long padded)
{
    long *l = c->beams.last;
    l[0] = kernel; l[1] = grid; l[2] = run; l[3] = nelem; l[4] = ntaps; l[5] = nbeams; l[6] = padded;
}

}  // namespace

int gpsiq_stap_beams_impl(gpsiq_ctx_t *c, int nelem, const void *const *src, const void *const *head, int nsamp, int sample_size,
                          const gpsiq_ctap_t *w, int ntaps, int nbeams, int shift, int out_sample_size, void *const *dst, void *hip_stream,
                          uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    // the sources and heads: gpsiq_stap_combine's checks, in its words
    if (nelem < 1 || nelem > kStapMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kStapMaxElem);
    if (ntaps < 1 || ntaps > kStapMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kStapMaxTaps);
    if (nelem * ntaps > kStapMaxRows) return fail(GPSIQ_E_ARG, "nelem %d * ntaps %d above %d rows", nelem, ntaps, kStapMaxRows);
    if (nbeams < 1 || nbeams > kBeamsMax) return fail(GPSIQ_E_ARG, "nbeams %d outside 1..%d", nbeams, kBeamsMax);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!src) return fail(GPSIQ_E_ARG, "null array of sources");
    if (!dst) return fail(GPSIQ_E_ARG, "null array of destinations");
    StapSources srcs;
    for (int e = 0; e < kStapMaxElem; ++e) { srcs.p[e] = nullptr; srcs.head[e] = nullptr; }
    for (int e = 0; e < nelem; ++e) {
        if (!src[e] && nsamp) return fail(GPSIQ_E_ARG, "null source %d", e);
        if ((uintptr_t) src[e] & 3) return fail(GPSIQ_E_ARG, "source %d %p not 4-byte aligned", e, src[e]);
        srcs.p[e] = static_cast<const uint8_t *>(src[e]);
        const void *h = head && ntaps > 1 ? head[e] : nullptr;        // (one tap reads nothing before the span)
        if ((uintptr_t) h & 3) return fail(GPSIQ_E_ARG, "head %d %p not 4-byte aligned", e, h);
        srcs.head[e] = static_cast<const uint8_t *>(h);
    }
    if (shift < 0 || shift > kStapMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kStapMaxShift);
    if (!w) return fail(GPSIQ_E_ARG, "null weights");
    const int rows = nelem * ntaps;
    const int16_t *re_im = &w[0].re;                                  // [nbeams][nelem][ntaps][2]: the struct is two int16 and no more
    int max_entry = -32768;
    for (int b = 0; b < nbeams; ++b) {
        const BeamsStats st = beams_weight_stats(re_im + 2 * (size_t) b * (size_t) rows, rows);
        if (st.mag > kStapWeightSum)
            return fail(GPSIQ_E_RANGE, "beam %d: sum |re| + |im| %ld above %ld: the accumulator would not hold the sum", b, st.mag, kStapWeightSum);
        if (st.max_entry > max_entry) max_entry = st.max_entry;
    }
    const size_t src_len = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, dst_len = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    const size_t head_len = (size_t) 2 * (size_t) (ntaps - 1) * (size_t) sample_size;
    BeamsDst dsts;
    for (int b = 0; b < kBeamsMax; ++b) dsts.p[b] = nullptr;
    for (int b = 0; b < nbeams; ++b) {
        if (!dst[b] && nsamp) return fail(GPSIQ_E_ARG, "null destination %d", b);
        if ((uintptr_t) dst[b] & 3) return fail(GPSIQ_E_ARG, "destination %d %p not 4-byte aligned", b, dst[b]);
        for (int e = 0; e < nelem; ++e) {
            if (overlap(dst[b], dst_len, src[e], src_len))
                return fail(GPSIQ_E_ARG, "source %d [%p, +%zu) and destination %d [%p, +%zu) overlap", e, src[e], src_len, b, dst[b], dst_len);
            if (srcs.head[e] && overlap(dst[b], dst_len, srcs.head[e], head_len))
                return fail(GPSIQ_E_ARG, "head %d [%p, +%zu) and destination %d [%p, +%zu) overlap", e, (const void *) srcs.head[e], head_len, b, dst[b], dst_len);
        }
        for (int a = 0; a < b; ++a)
            if (overlap(dst[b], dst_len, dst[a], dst_len))
                return fail(GPSIQ_E_ARG, "destinations %d [%p, +%zu) and %d [%p, +%zu) overlap", a, dst[a], dst_len, b, dst[b], dst_len);
        dsts.p[b] = static_cast<uint8_t *>(dst[b]);
    }
    if (clipped) std::memset(clipped, 0, sizeof(uint64_t) * (size_t) nbeams);
    if (kernel_ms) *kernel_ms = 0.0f;
    const BeamsPlan p = plan_stap_beams(nelem, ntaps, nbeams, nsamp, sample_size, out_sample_size, max_entry, forced_kernel("GPSIQ_STAP_BEAMS_KERNEL", "mfma"));
    note_plan(c, -1, 0, 0, nelem, ntaps, nbeams, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    BeamsSet &k = c->beams;
    if (int rc = k.reserve()) return rc;
    const BeamsFn kernel = p.kernel == kBeamsMfma ? stap_beams_mfma_kernel(sample_size, out_sample_size, p.padded) : stap_beams_generic_kernel(sample_size, out_sample_size);
    if (!kernel)
        return fail(GPSIQ_E_DEVICE, "no beams kernel %d for %d-byte samples to %d-byte outputs with %d padded taps", p.kernel, sample_size, out_sample_size, p.padded);
    // Nothing queued earlier still reads h_coef or h_count: every call ends synchronised
    beams_build_coef(re_im, nelem, ntaps, nbeams, p.padded, k.h_coef.get());
    HIP_TRY(hipMemcpyAsync(k.d_coef.get(), k.h_coef.get(), sizeof(uint32_t) * kBeamsCoefDwords, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(k.d_count.get(), 0, sizeof(unsigned long long) * kBeamsMax, s));     // the workgroups add into them: zeroed per call
    HIP_TRY(hipEventRecord(k.t0.get(), s));
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, srcs, k.d_coef.get(), nelem, ntaps, nbeams, nsamp, shift, dsts, p.runs, k.d_count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(k.t1.get(), s));
    HIP_TRY(hipMemcpyAsync(k.h_count.get(), k.d_count.get(), sizeof(unsigned long long) * kBeamsMax, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (clipped)
        for (int b = 0; b < nbeams; ++b) clipped[b] = (uint64_t) k.h_count[b];
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.t0.get(), k.t1.get()));
    note_plan(c, p.kernel, (long) p.grid, (long) p.run, nelem, ntaps, nbeams, p.padded);
    return GPSIQ_OK;
}

extern "C" int gpsiq_stap_beams_last_plan(const gpsiq_ctx_t *c, long out[7])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 7; ++i) out[i] = c->beams.last[i];
    return GPSIQ_OK;
}
