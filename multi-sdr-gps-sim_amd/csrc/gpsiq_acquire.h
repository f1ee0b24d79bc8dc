// gpsiq_acquire.h -- what the device context holds for gpsiq_acquire (include/gpsiq_rows.h, "Acquisition") and what its host side
// (gpsiq_acquire.cpp) and its kernels (gpsiq_acquire_kernels.hip, with gpsiq_acquire_geometry.h) use of each other.  The plan is in
// gpsiq_acquire_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `acq`.
#ifndef GPSIQ_ACQUIRE_H
#define GPSIQ_ACQUIRE_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// the satellite list, the power grid, the peaks and (where the caller asks for them) the correlations of one call on the device, the
// digit planes of the matrix path, the page-locked staging of list and peaks (grid and correlations cross straight into the caller's
// arrays), and the events the kernels are timed with
struct AcquireSet {
    DevBuf<uint8_t>                 d_prn;    PinnedBuf<uint8_t>              h_prn;        // [nprn]
    DevBuf<double>                  d_power;                                                // [nprn][ndopp][nshift]
    DevBuf<gpsiq_acquire_peak_t>    d_peaks;  PinnedBuf<gpsiq_acquire_peak_t> h_peaks;      // [nprn][ndopp]
    DevBuf<gpsiq_despread_sum_t>    d_corr;                                                 // [nprn][ndopp][nnoncoh][nshift]
    DevBuf<uint8_t>                 d_planes;                                               // bytes (gpsiq_acquire_plan.h: scratch_bytes)
    Event          t0, t1, t2;                      // before stage one, between the stages, behind the peaks
    long long      last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, scratch bytes, grid of the main kernel, k-steps
    float          last_ms[2] = {0.0f, 0.0f};       // the last call's device time: stage one (0 for the generic kernel), the rest
    // first use + room for one call (corr_cells 0: the correlations are not asked for; plane_bytes 0: the generic kernel)
    int reserve(size_t cells, size_t peaks, size_t corr_cells, size_t plane_bytes);
};

// (the satellite list, events and peaks on first use; the peaks' pair grows together, device side first)
inline int AcquireSet::reserve(size_t cells, size_t npeaks, size_t corr_cells, size_t plane_bytes)
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(t2.ensure(hipEventDefault));
    HIP_TRY(d_prn.reserve(32));
    HIP_TRY(h_prn.reserve(32));
    HIP_TRY(reserve_together(cells, cells + cells / 4 + 256, d_power));
    HIP_TRY(reserve_together(npeaks, npeaks + npeaks / 4 + 64, d_peaks, h_peaks));
    HIP_TRY(reserve_together(corr_cells, corr_cells + corr_cells / 4 + 256, d_corr));
    HIP_TRY(reserve_together(plane_bytes, plane_bytes + plane_bytes / 4 + 256, d_planes));
    return GPSIQ_OK;
}

// the acquisition kernels (gpsiq_acquire_kernels.hip).  generic: stream, tables, satellites, nshift, ncoh, nnoncoh, hop, ndopp, code step,
// carrier step of bin 0 and between bins (mod 2^64), power grid, correlations (may be null).  wipe: stream, tables, span, plane length,
// ndopp, row tiles, the carrier steps, planes.  mfma: planes, tables, satellites, plane length, row tiles, nshift, ncoh, nnoncoh, hop,
// ndopp, code step, k-steps, power grid, correlations (may be null).  peaks: power grid, its rows, nshift, peaks
using AcquireGenericFn = void (*)(const uint8_t *, const DeviceTables *, const uint8_t *, int, int, int, int, int, uint64_t, uint64_t, uint64_t,
                                  double *, gpsiq_despread_sum_t *);
using AcquireWipeFn    = void (*)(const uint8_t *, const DeviceTables *, uint64_t, uint64_t, int, int, uint64_t, uint64_t, uint8_t *);
using AcquireMfmaFn    = void (*)(const uint8_t *, const DeviceTables *, const uint8_t *, uint64_t, int, int, int, int, int, int, uint64_t, int,
                                  double *, gpsiq_despread_sum_t *);
using AcquirePeaksFn   = void (*)(const double *, uint64_t, int, gpsiq_acquire_peak_t *);
AcquireGenericFn acquire_generic_kernel(int fmt);
AcquireWipeFn    acquire_wipe_kernel(int fmt);
AcquireMfmaFn    acquire_mfma_kernel(int digits);
AcquirePeaksFn   acquire_peaks_kernel();

}  // namespace gpsiq

// gpsiq_acquire.cpp: gpsiq_acquire itself, behind the plumbing entry "acquire".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_acquire) gpsiq_acquire_impl;
#endif
