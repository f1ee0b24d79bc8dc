// gpsiq_acquire.cpp -- host side of gpsiq_acquire (include/gpsiq_rows.h, "Acquisition"): checks, plan (gpsiq_acquire_plan.h, pure and
// pinned on the CPU), kernel look-up (gpsiq_acquire_kernels.hip holds the kernels and the table of those that exist), scratch, launch,
// copy-back.  libgpsiq_rows.so exports the typed call and reaches this through the plumbing entry "acquire".  Host code: nothing here
// decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_acquire.h"
#include "gpsiq_acquire_plan.h"

using namespace gpsiq;

// the words and codes of gpsiq_launch's checks (check_launch, gpsiq_device.cpp), for a source instead of a destination
static int check_acquire(const gpsiq_ctx *c, int nsamp, int sample_size, const void *src, const uint8_t *prn, int nprn, int ndopp, int nshift,
                         int ncoh, int nnoncoh, int hop, const void *peaks)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (ncoh < 64 || ncoh > kAcqMaxNcoh || (ncoh & 63)) return fail(GPSIQ_E_ARG, "coherent length %d: a multiple of 64, from 64 to %d", ncoh, kAcqMaxNcoh);
    if (nshift < 1 || nnoncoh < 1 || hop < 1) return fail(GPSIQ_E_ARG, "shifts %d, dwells %d, hop %d: each at least 1", nshift, nnoncoh, hop);
    if (ndopp < 1 || ndopp > kAcqMaxDopp) return fail(GPSIQ_E_ARG, "%d Doppler bins: 1 to %d", ndopp, kAcqMaxDopp);
    if (nprn < 1 || nprn > kAcqMaxPrn) return fail(GPSIQ_E_ARG, "%d satellites: 1 to %d", nprn, kAcqMaxPrn);
    if (!prn || !peaks) return fail(GPSIQ_E_ARG, "null argument");
    for (int p = 0; p < nprn; ++p)
        if (prn[p] < 1 || prn[p] > 32) return fail(GPSIQ_E_ARG, "prn %d out of range 1..32", (int) prn[p]);
    const int64_t span = ((int64_t) nshift - 1) + ((int64_t) nnoncoh - 1) * (int64_t) hop + (int64_t) ncoh;      // every factor below 2^31
    if (span > (int64_t) nsamp) return fail(GPSIQ_E_ARG, "the search reads %lld samples, the stream has %d", (long long) span, nsamp);
    if (!src) return fail(GPSIQ_E_ARG, "null source");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    return GPSIQ_OK;
}

int gpsiq_acquire_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, void *hip_stream, const uint8_t *prn, int nprn,
                       uint64_t code_step, int64_t carr_step0, int64_t carr_step_inc, int ndopp, int nshift, int ncoh, int nnoncoh, int hop,
                       gpsiq_acquire_peak_t *peaks, double *power, gpsiq_despread_sum_t *corr, float *kernel_ms)
{
    if (c) { c->acq.last[0] = -1; c->acq.last[1] = c->acq.last[2] = c->acq.last[3] = 0; c->acq.last_ms[0] = c->acq.last_ms[1] = 0.0f; }
    if (int rc = check_acquire(c, nsamp, sample_size, src, prn, nprn, ndopp, nshift, ncoh, nnoncoh, hop, peaks)) return rc;
    if (kernel_ms) *kernel_ms = 0.0f;
    const char *force = std::getenv("GPSIQ_ACQUIRE_KERNEL");
    const AcquirePlan p = plan_acquire(nsamp, sample_size, nprn, ndopp, nshift, ncoh, nnoncoh, hop, force && !std::strcmp(force, "generic"),
                                       kAcqFastDefault, force && !std::strcmp(force, "mfma"));
    AcquireSet &a = c->acq;
    if (p.kind != kPlanLaunch) return fail(GPSIQ_E_ARG, "not a search");       // (the checks above and the planner's are the same list)
    const bool fast = p.kernel == kAcquireMfma;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    const size_t npeaks = (size_t) nprn * (size_t) ndopp;
    if (int rc = a.reserve((size_t) p.cells, npeaks, corr ? (size_t) p.corr_cells : 0, fast ? (size_t) p.scratch_bytes : 0)) return rc;
    const AcquirePeaksFn peaks_kernel = acquire_peaks_kernel();
    const AcquireGenericFn generic = acquire_generic_kernel(sample_size);
    const AcquireWipeFn wipe = acquire_wipe_kernel(sample_size);
    const AcquireMfmaFn mfma = acquire_mfma_kernel(p.digits);
    if (!peaks_kernel || (fast ? !wipe || !mfma : !generic))
        return fail(GPSIQ_E_DEVICE, "no acquisition kernel %s for %d-byte samples", acquire_kernel_name(p.kernel), sample_size);

    std::memcpy(a.h_prn.get(), prn, (size_t) nprn);
    HIP_TRY(hipMemcpyAsync(a.d_prn.get(), a.h_prn.get(), (size_t) nprn, hipMemcpyHostToDevice, s));
    const uint8_t *stream = static_cast<const uint8_t *>(src);
    gpsiq_despread_sum_t *d_corr = corr ? a.d_corr.get() : nullptr;
    HIP_TRY(hipEventRecord(a.t0.get(), s));
    if (fast) {
        hipLaunchKernelGGL(wipe, dim3((unsigned) p.wipe_grid), dim3(kAcqThreads), 0, s, stream, c->d_tab.get(), p.span, p.npad, ndopp, p.row_tiles,
                           (uint64_t) carr_step0, (uint64_t) carr_step_inc, a.d_planes.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(a.t1.get(), s));
        hipLaunchKernelGGL(mfma, dim3(p.mx, p.my, p.mz), dim3(kAcqWaves * 64), p.lds_bytes, s, a.d_planes.get(), c->d_tab.get(), a.d_prn.get(), p.npad,
                           p.row_tiles, nshift, ncoh, nnoncoh, hop, ndopp, code_step, p.ksteps, a.d_power.get(), d_corr);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipEventRecord(a.t1.get(), s));
        hipLaunchKernelGGL(generic, dim3(p.gx, p.gy, p.gz), dim3(kAcqThreads), 0, s, stream, c->d_tab.get(), a.d_prn.get(), nshift, ncoh, nnoncoh, hop,
                           ndopp, code_step, (uint64_t) carr_step0, (uint64_t) carr_step_inc, a.d_power.get(), d_corr);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(peaks_kernel, dim3((unsigned) p.peak_grid), dim3(kAcqThreads), 0, s, a.d_power.get(), (uint64_t) npeaks, nshift, a.d_peaks.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(a.t2.get(), s));
    HIP_TRY(hipMemcpyAsync(a.h_peaks.get(), a.d_peaks.get(), npeaks * sizeof(gpsiq_acquire_peak_t), hipMemcpyDeviceToHost, s));
    if (power) HIP_TRY(hipMemcpyAsync(power, a.d_power.get(), (size_t) p.cells * sizeof(double), hipMemcpyDeviceToHost, s));
    if (corr) HIP_TRY(hipMemcpyAsync(corr, a.d_corr.get(), (size_t) p.corr_cells * sizeof(gpsiq_despread_sum_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(peaks, a.h_peaks.get(), npeaks * sizeof(gpsiq_acquire_peak_t));
    HIP_TRY(hipEventElapsedTime(&a.last_ms[0], a.t0.get(), a.t1.get()));
    HIP_TRY(hipEventElapsedTime(&a.last_ms[1], a.t1.get(), a.t2.get()));
    if (kernel_ms) *kernel_ms = a.last_ms[0] + a.last_ms[1];
    a.last[0] = p.kernel; a.last[1] = (long long) p.scratch_bytes;
    a.last[2] = fast ? (long long) p.mx * p.my * p.mz : (long long) p.gx * p.gy * p.gz; a.last[3] = p.ksteps;
    return GPSIQ_OK;
}

extern "C" int gpsiq_acquire_last_plan(const gpsiq_ctx_t *c, long long out[4], float ms[2])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->acq.last[i];
    if (ms) { ms[0] = c->acq.last_ms[0]; ms[1] = c->acq.last_ms[1]; }
    return GPSIQ_OK;
}
