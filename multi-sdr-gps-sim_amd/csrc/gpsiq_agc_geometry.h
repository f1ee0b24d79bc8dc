// gpsiq_agc_geometry.h -- the geometry the AGC kernels (gpsiq_agc_kernels.hip) are compiled for and the planner (gpsiq_agc_plan.h)
// cuts its grids by, the ranges of the contract (include/gpsiq_rows.h, "AGC") and the gain rule itself, which the gains kernel and
// gpsiq_agc_mult (gpsiq_stage_math.cpp) both evaluate from here.  These decide device code, so the file is one of the device sources
// behind gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants and integer arithmetic: host and device code include it alike.
#ifndef GPSIQ_AGC_GEOMETRY_H
#define GPSIQ_AGC_GEOMETRY_H

#include <cstdint>

#if defined(__HIPCC__)
#define GPSIQ_AGC_HD __host__ __device__
#else
#define GPSIQ_AGC_HD
#endif

namespace gpsiq {

constexpr int kAgcThreads = 256;               // four waves per workgroup, every kernel
// A UNIT is the 8 consecutive samples one lane loads in one go: 16 bytes of int8, two loads of 16 bytes of int16 -- and one byte of
// the blank mask.  A unit is wide only where all of it lies inside the span; the one ragged unit at the span's end goes element by
// element.
constexpr int kAgcUnit = 8;
constexpr int kAgcTile = kAgcThreads * kAgcUnit;           // agc_measure: samples of a workgroup's tile, one unit per lane
constexpr int kAgcApplyUnits = 2;                          // agc_apply: units per lane, kAgcThreads apart
constexpr int kAgcApplyTile = kAgcTile * kAgcApplyUnits;   // samples of a workgroup
// the ranges of the contract
constexpr int kAgcMinWindow = 64, kAgcMaxWindow = 65536, kAgcMaxAvg = 64, kAgcMaxHold = 1024, kAgcMaxThresh = 32767;
constexpr uint32_t kAgcMaxTarget = (1u << 23) - 1, kAgcMaxMult = (1u << 24) - 1;
constexpr uint64_t kAgcMaxSum = UINT64_C(1) << 53, kAgcMaxCount = UINT64_C(1) << 23;
// a tile touches at most kAgcTile / kAgcMinWindow + 1 windows: the slots a workgroup reduces into before its atomics
constexpr int kAgcTileWindows = kAgcTile / kAgcMinWindow + 1;
// agc_measure reads the blank_hold samples in front of its tile again, in whole units: at most this many lanes of lead-in
constexpr int kAgcLeadUnits = kAgcMaxHold / kAgcUnit;
static_assert(kAgcLeadUnits <= kAgcThreads, "the lead-in is read in one step");

// floor square root of m < 2^63
GPSIQ_AGC_HD inline uint64_t agc_isqrt(uint64_t m)
{
    uint64_t r = 0;
    for (uint64_t bit = UINT64_C(1) << 31; bit; bit >>= 1) {
        const uint64_t t = r | bit;
        if (t * t <= m) r = t;
    }
    return r;
}

// The gain rule: S = sumsq <= 2^53 over n = count <= 2^23 elements.  m = floor(S * 2^16 / n) in two divisions that stay inside 64
// bits, r = max(isqrt(m), 1) the rms in 1/256 units, the multiplier floor((target_q8 << 16) / r) between its clamps
GPSIQ_AGC_HD inline uint32_t agc_gain(uint64_t sumsq, uint64_t count, uint32_t target_q8, uint32_t mult0, uint32_t mult_min, uint32_t mult_max)
{
    if (count == 0) return mult0;
    const uint64_t m = ((sumsq / count) << 16) + (((sumsq % count) << 16) / count);
    uint64_t r = agc_isqrt(m);
    if (r < 1) r = 1;
    const uint64_t g = ((uint64_t) target_q8 << 16) / r;
    return g < mult_min ? mult_min : g > mult_max ? mult_max : (uint32_t) g;
}

}  // namespace gpsiq
#endif
