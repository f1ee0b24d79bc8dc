// gpsiq_follow_geometry.h -- the geometry the follow kernel (gpsiq_follow_kernels.hip) is compiled for and the planner
// (gpsiq_follow_plan.h) cuts its grid by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain C++: the planner compiles without HIP.
#ifndef GPSIQ_FOLLOW_GEOMETRY_H
#define GPSIQ_FOLLOW_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kFollowWaves = 4;                    // waves of a workgroup: one workgroup serves one satellite
constexpr int kFollowThreads = kFollowWaves * 64;
constexpr int kFollowRow = 64;                     // samples of a row: one per lane; the waves take an epoch's rows in turn
constexpr int kFollowSums = 6;                     // Ie, Qe, Ip, Qp, Il, Ql
constexpr int kFollowMaxEpochLen = 16368;          // 1023 * 2^56 / 2^52: the longest epoch the range of the code step allows

}  // namespace gpsiq
#endif
