// gpsiq_stap_beams.h -- what the device context holds for gpsiq_stap_beams (include/gpsiq_rows.h, "Space-time array") and what its host
// side (gpsiq_stap_beams.cpp) and its kernels (gpsiq_stap_beams_kernels.hip, with gpsiq_stap_beams_geometry.h) use of each other.  The
// plan is in gpsiq_stap_beams_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `beams`.
#ifndef GPSIQ_STAP_BEAMS_H
#define GPSIQ_STAP_BEAMS_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_stap.h"
#include "gpsiq_stap_beams_geometry.h"

namespace gpsiq {

static_assert(kBeamsMax == GPSIQ_STAP_MAX_BEAMS, "the geometry's size is the contract's");

// the destinations of a call as the kernels take them: by value, in the argument block, wave-uniform
struct BeamsDst { uint8_t *p[kBeamsMax]; };

// the coefficients of a call (the matrix kernel's planes and row constants, the generic kernel's weights: kBeamsCoefDwords dwords) and
// the counters of clamped elements, one per beam, each on the device and page-locked on its way there or back; the two timing events
struct BeamsSet {
    DevBuf<uint32_t>              d_coef;    PinnedBuf<uint32_t>           h_coef;        // [kBeamsCoefDwords]
    DevBuf<unsigned long long>    d_count;   PinnedBuf<unsigned long long> h_count;       // [kBeamsMax]
    Event          t0, t1;
    long           last[7] = {-1, 0, 0, 0, 0, 0, 0};      // the last call's plan: kernel, grid, run, elements, taps, beams, padded taps
    int reserve();                                          // first use
};

inline int BeamsSet::reserve()
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(reserve_together(kBeamsCoefDwords, kBeamsCoefDwords, d_coef, h_coef));
    HIP_TRY(reserve_together(kBeamsMax, kBeamsMax, d_count, h_count));
    return GPSIQ_OK;
}

// the stage's kernels (gpsiq_stap_beams_kernels.hip).  Both: streams and heads, the coefficients, elements, taps, beams, samples, shift,
// the destinations, the runs of the span (gpsiq_stap_beams_plan.h), the counters (zeroed by the host)
using BeamsFn = void (*)(const StapSources, const uint32_t *, int, int, int, int, int, const BeamsDst, uint64_t, unsigned long long *);
BeamsFn stap_beams_generic_kernel(int in_fmt, int out_fmt);
BeamsFn stap_beams_mfma_kernel(int in_fmt, int out_fmt, int padded_taps);

}  // namespace gpsiq

// gpsiq_stap_beams.cpp: the call itself, behind the plumbing entry "stap_beams".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_stap_beams) gpsiq_stap_beams_impl;
#endif
