// gpsiq_mix.h -- what the device context holds for gpsiq_mix / gpsiq_generate_batch_mixed (include/gpsiq_rows.h, "Mix") and what their
// host side (gpsiq_mix.cpp) and their kernels (gpsiq_mix_kernels.hip, with gpsiq_mix_geometry.h) use of each other.  The plan is in
// gpsiq_mix_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `mix`.
#ifndef GPSIQ_MIX_H
#define GPSIQ_MIX_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_mix_geometry.h"

namespace gpsiq {

// the carrier table as the kernels read it (512 dwords: cos below, sin above) on the device (have: it has arrived) and page-locked on
// its way there, and the counter of clamped elements with its timing events (gpsiq_stage_call.h).  The batch call works through its
// pieces with the context's staging ring (gpsiq_stage_batch.h), in place in the rendered pair
struct MixSet {
    DevBuf<uint32_t>              d_table;   PinnedBuf<uint32_t>           h_table;       // [512]
    bool                          have_table = false;
    ClipCount      clip;
    long long      last[4] = {-1, 0, 0, 0};         // the last call's plan: kernel, grid, units, pieces (gpsiq_mix_last_plan)
    int reserve();                                  // first use
};

inline int MixSet::reserve()
{
    if (int rc = clip.reserve()) return rc;
    HIP_TRY(reserve_together(512, 512, d_table, h_table));
    return GPSIQ_OK;
}

// the mix kernels (gpsiq_mix_kernels.hip).  Arguments: the terms, m0, the samples, shift, qmax, destination; row kernel: the samples
// of the first slot before sample 0 and the slots of the launch (gpsiq_mix_plan.h); the table; the counter of clamped elements
using MixGenericFn = void (*)(const MixDevTerms, uint64_t, int, int, int, uint8_t *, const uint32_t *, unsigned long long *);
using MixRowsFn    = void (*)(const MixDevTerms, uint64_t, int, int, int, uint8_t *, int, uint64_t, const uint32_t *, unsigned long long *);
MixGenericFn mix_generic_kernel(int out_fmt);
MixRowsFn    mix_rows_kernel(int out_fmt);

}  // namespace gpsiq

// gpsiq_mix.cpp: gpsiq_mix and gpsiq_generate_batch_mixed themselves, behind the plumbing entries "mix" and "generate_batch_mixed".
// Declared from the public prototypes, and hidden: a definition that has drifted from include/gpsiq_rows.h is another function, and
// the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_mix) gpsiq_mix_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_generate_batch_mixed) gpsiq_generate_batch_mixed_impl;
#endif
