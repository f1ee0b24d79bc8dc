// gpsiq_follow_plan.h -- how a gpsiq_follow call (include/gpsiq_rows.h, "Follow") is cut into launches, and which of its arguments are
// a call at all.  Host code only, and pure: no HIP, no environment (the knob is an argument).  tests/follow_plan.cpp pins every plan
// on the CPU.  Not a device source: the geometry the kernel is compiled for is gpsiq_follow_geometry.h, the list of kernels that
// exist is in gpsiq_follow_kernels.hip.
// The loop is serial in time per satellite, so the grid is one workgroup per satellite and nothing else; what the planner owns is the
// bound on a launch: at most epochs_per_launch epochs per satellite, after which the host relaunches from the device-resident state
// until every satellite has stopped.  A launch is therefore bounded whatever the span, and the relaunch is the same path as a caller
// continuing from a returned state.
#ifndef GPSIQ_FOLLOW_PLAN_H
#define GPSIQ_FOLLOW_PLAN_H

#include <cstdint>

#include "gpsiq_follow_geometry.h"
#include "gpsiq_launch_plan.h"

namespace gpsiq {

constexpr int kFollowMaxPrn = 32;
constexpr int kFollowEpochsPerLaunch = 4096;       // about 4 s of stream per launch at the nominal code rate
constexpr uint64_t kFollowRecordBytes = 96;        // sizeof(gpsiq_follow_epoch_t)
constexpr uint64_t kFollowRecordCap = UINT64_C(1) << 30;      // bytes of records a call may ask for

struct FollowPlan {
    int      kind = kPlanNothing;      // kPlanNothing: the arguments are not a call (nothing is launched) | kPlanLaunch
    unsigned grid = 0;                 // workgroups: one per satellite
    unsigned threads = 0;
    int      epochs_per_launch = 0;
    uint64_t records = 0;              // nprn * max_epochs
    uint64_t record_bytes = 0;
    int      max_launches = 0;         // launches the call can take at most: see follow_launches
};

// the value of GPSIQ_FOLLOW_EPOCHS_PER_LAUNCH as the call takes it: anything outside 1..kFollowEpochsPerLaunch is the default
inline int follow_epochs_per_launch(int64_t knob) { return knob >= 1 && knob <= kFollowEpochsPerLaunch ? (int) knob : kFollowEpochsPerLaunch; }

// launches a satellite that ends with `records` records takes: the launch in which it stops does records % per_launch epochs first,
// and a satellite that has done exactly per_launch epochs in a launch is seen to stop only by the next one
inline int follow_launches(int64_t records, int per_launch) { return (int) (records / per_launch) + 1; }

inline bool follow_args_ok(int64_t nsamp, int sample_size, int nprn, int64_t max_epochs)
{
    if (sample_size != 1 && sample_size != 2) return false;
    if (nsamp < 0 || nsamp > INT32_MAX || nprn < 1 || nprn > kFollowMaxPrn || max_epochs < 1 || max_epochs > INT32_MAX) return false;
    return (uint64_t) nprn * (uint64_t) max_epochs * kFollowRecordBytes <= kFollowRecordCap;
}

inline FollowPlan plan_follow(int64_t nsamp, int sample_size, int nprn, int64_t max_epochs, int64_t knob = 0)
{
    FollowPlan p;
    if (!follow_args_ok(nsamp, sample_size, nprn, max_epochs)) return p;
    p.kind = kPlanLaunch;
    p.grid = (unsigned) nprn;
    p.threads = kFollowThreads;
    p.epochs_per_launch = follow_epochs_per_launch(knob);
    p.records = (uint64_t) nprn * (uint64_t) max_epochs;
    p.record_bytes = p.records * kFollowRecordBytes;
    // a satellite writes at most min(max_epochs, nsamp) records: an epoch is at least one sample
    p.max_launches = follow_launches(max_epochs < nsamp ? max_epochs : nsamp, p.epochs_per_launch);
    return p;
}

}  // namespace gpsiq
#endif
