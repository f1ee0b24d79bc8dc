// gpsiq_pack.h -- what the device context holds for gpsiq_pack / gpsiq_unpack / gpsiq_generate_batch_packed (include/gpsiq_rows.h,
// "Packed streams") and what their host side (gpsiq_pack.cpp) and their kernels (gpsiq_pack_kernels.hip, with gpsiq_pack_geometry.h)
// use of each other.  The plan is in gpsiq_pack_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `pack`.
#ifndef GPSIQ_PACK_H
#define GPSIQ_PACK_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_stage_call.h"

namespace gpsiq {

// the counter of clamped elements with its timing events (gpsiq_stage_call.h; gpsiq_unpack uses the events alone).  The batch call
// works through its pieces with the context's staging ring (gpsiq_stage_batch.h)
struct PackSet {
    ClipCount      clip;
    long           last[4] = {-1, 0, 0, 0};         // the last call's plan: grid, units per block, tiles per block, pieces (gpsiq_pack_last_plan)
    int reserve() { return clip.reserve(); }        // first use
};

// the pack / unpack kernels (gpsiq_pack_kernels.hip).  Arguments: source and its block stride, destination and its block stride,
// samples per block, units per block, tiles per block, tiles of the launch (gpsiq_pack_plan.h); pack: the counter of clamped elements
using PackFn      = void (*)(const uint8_t *, size_t, uint8_t *, size_t, int, uint32_t, uint32_t, uint64_t, unsigned long long *);
using UnpackFn    = void (*)(const uint8_t *, size_t, uint8_t *, size_t, int, uint32_t, uint32_t, uint64_t);
PackFn      pack_kernel(int fmt, int bits);
UnpackFn    unpack_kernel(int bits, int fmt);

}  // namespace gpsiq

// gpsiq_pack.cpp: gpsiq_pack, gpsiq_unpack and gpsiq_generate_batch_packed themselves, behind the plumbing entries "pack", "unpack"
// and "generate_batch_packed".  Declared from the public prototypes, and hidden: a definition that has drifted from
// include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_pack) gpsiq_pack_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_unpack) gpsiq_unpack_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_generate_batch_packed) gpsiq_generate_batch_packed_impl;
#endif
