// gpsiq_follow.h -- what the device context holds for gpsiq_follow (include/gpsiq_rows.h, "Follow") and what its host side
// (gpsiq_follow.cpp) and its kernel (gpsiq_follow_kernels.hip, with gpsiq_follow_geometry.h) use of each other.  The plan is in
// gpsiq_follow_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `fol`.
#ifndef GPSIQ_FOLLOW_H
#define GPSIQ_FOLLOW_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// the satellites' states and record counts on the device and page-locked on their way there and back, the records on the device (they
// cross straight into the caller's array), and the events a launch is timed with
struct FollowSet {
    DevBuf<gpsiq_follow_state_t>    d_state;  PinnedBuf<gpsiq_follow_state_t> h_state;      // [nprn]
    DevBuf<int>                     d_count;  PinnedBuf<int>                  h_count;      // [nprn]
    DevBuf<gpsiq_follow_epoch_t>    d_epochs;                                               // [nprn][max_epochs]
    Event          t0, t1;
    long long      last[4] = {-1, 0, 0, 0};         // the last call's plan: grid, epochs per launch, launches, bytes of records
    int reserve(size_t records);                    // first use + room for one call
};

// (states, counts and events on first use; the records grow)
inline int FollowSet::reserve(size_t records)
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(d_state.reserve(32));
    HIP_TRY(h_state.reserve(32));
    HIP_TRY(d_count.reserve(32));
    HIP_TRY(h_count.reserve(32));
    HIP_TRY(reserve_together(records, records + records / 4 + 64, d_epochs));
    return GPSIQ_OK;
}

// the follow kernel (gpsiq_follow_kernels.hip): stream, its samples, tables, configuration, states, records, records per satellite,
// record counts, epochs this launch does per satellite at most
using FollowFn = void (*)(const uint8_t *, uint64_t, const DeviceTables *, gpsiq_follow_cfg_t, gpsiq_follow_state_t *, gpsiq_follow_epoch_t *, int,
                          int *, int);
FollowFn follow_kernel(int fmt);

}  // namespace gpsiq

// gpsiq_follow.cpp: gpsiq_follow itself, behind the plumbing entry "follow".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_follow) gpsiq_follow_impl;
#endif
