// gpsiq_pack.h -- what the device context holds for gpsiq_pack / gpsiq_unpack / gpsiq_generate_batch_packed (include/gpsiq_rows.h,
// "Packed streams") and what their host side (gpsiq_pack.cpp) and their kernels (gpsiq_pack_kernels.hip, with gpsiq_pack_geometry.h)
// use of each other.  The plan is in gpsiq_pack_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `pack`.
#ifndef GPSIQ_PACK_H
#define GPSIQ_PACK_H

#include <vector>

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// the counter of clamped elements on the device and page-locked on its way back, the two events a kernel is timed with, and what the
// batch call works through its pieces with -- two rendered and two packed staging buffers taken in turn, a stream for the packer,
// one for the copies, and per buffer pair the events "packed" and "copied"
struct PackSet {
    DevBuf<unsigned long long>    d_count;   PinnedBuf<unsigned long long> h_count;       // [1]
    DevBuf<uint8_t>               d_render[2], d_packed[2];                               // bytes
    Stream         pack_stream, copy_stream;
    Event          t0, t1, packed[2], copied[2];
    std::vector<gpsiq_chan_t> row;                  // a piece's descriptors with the carrier phases handed over in its first block
    long           last[4] = {-1, 0, 0, 0};         // the last call's plan: grid, units per block, tiles per block, pieces (gpsiq_pack_last_plan)
    int reserve(size_t render_bytes, size_t packed_bytes);      // first use + room for one call (0, 0: gpsiq_pack / gpsiq_unpack)
};

// (the counter, events and streams on first use; the staging pairs grow together, rendered side first)
inline int PackSet::reserve(size_t render_bytes, size_t packed_bytes)
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(d_count.reserve(1));
    HIP_TRY(h_count.reserve(1));
    if (!render_bytes && !packed_bytes) return GPSIQ_OK;
    HIP_TRY(pack_stream.ensure());
    HIP_TRY(copy_stream.ensure());
    for (auto &e : packed) HIP_TRY(e.ensure());
    for (auto &e : copied) HIP_TRY(e.ensure());
    HIP_TRY(reserve_together(render_bytes, render_bytes + render_bytes / 4 + 256, d_render[0], d_render[1]));
    HIP_TRY(reserve_together(packed_bytes, packed_bytes + packed_bytes / 4 + 256, d_packed[0], d_packed[1]));
    return GPSIQ_OK;
}

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
