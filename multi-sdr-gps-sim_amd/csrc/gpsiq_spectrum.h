// gpsiq_spectrum.h -- what the device context holds for gpsiq_spectrum (include/gpsiq_rows.h, "Spectrum") and what its host side
// (gpsiq_spectrum.cpp) and its kernels (gpsiq_spectrum_kernels.hip, with gpsiq_spectrum_geometry.h) use of each other.  The plan is in
// gpsiq_spectrum_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `spec`.
#ifndef GPSIQ_SPECTRUM_H
#define GPSIQ_SPECTRUM_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_spectrum_geometry.h"

namespace gpsiq {

// the carrier table as the generic kernel reads it (512 dwords: cos below, sin above) on the device and page-locked on its way there;
// the matrix kernel's table matrix, one per (nfft, window), built on the host ONCE in fragment order, kept on the device (have: it has
// arrived) and page-locked on its way there (one size: the largest); the device result and its page-locked twin, which grow together;
// the two events the kernels are timed with
struct SpectrumSet {
    static constexpr int kMats = 8;                  // (log2(nfft) - 6) * 2 + window
    DevBuf<uint32_t>            d_table;   PinnedBuf<uint32_t>           h_table;       // [512]
    bool                        have_table = false;
    DevBuf<uint8_t>             d_mat[kMats];
    bool                        have_mat[kMats] = {};
    PinnedBuf<uint8_t>          h_mat;                                                   // [2 * spectrum_plane_bytes(kSpecMaxFft)]
    DevBuf<unsigned long long>  d_power;   PinnedBuf<unsigned long long> h_power;       // [ngroups * nfft]
    Event          t0, t1;
    long long      last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, segments of a unit / pass, groups (gpsiq_spectrum_last_plan)
    int reserve(size_t cells);                      // first use + room for one call's result
};

inline int SpectrumSet::reserve(size_t cells)
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(reserve_together(512, 512, d_table, h_table));
    HIP_TRY(reserve_together(cells, cells + cells / 4 + 512, d_power, h_power));
    return GPSIQ_OK;
}

// the spectrum kernels (gpsiq_spectrum_kernels.hip).  Generic: span, table, nfft, hop, window, shift, navg, units of a group, units of
// the launch, power.  Matrix: span, digit planes, nfft, hop, shift, navg, segments read, segments of a pass, passes of the launch and
// of a workgroup, power (gpsiq_spectrum_plan.h)
using SpectrumGenericFn = void (*)(const uint8_t *, const uint32_t *, int, int, int, int, int, uint64_t, uint64_t, unsigned long long *);
using SpectrumMfmaFn    = void (*)(const uint8_t *, const uint8_t *, int, int, int, int, uint32_t, int, uint64_t, uint64_t, unsigned long long *);
SpectrumGenericFn spectrum_generic_kernel(int fmt);
SpectrumMfmaFn    spectrum_mfma_kernel(int fmt);

}  // namespace gpsiq

// gpsiq_spectrum.cpp: gpsiq_spectrum itself, behind the plumbing entry "spectrum".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_spectrum) gpsiq_spectrum_impl;
#endif
