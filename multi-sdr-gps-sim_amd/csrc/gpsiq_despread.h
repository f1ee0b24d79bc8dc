// gpsiq_despread.h -- what the device context holds for gpsiq_despread (include/gpsiq_rows.h, "Despread") and what its host side
// (gpsiq_despread.cpp) and its kernels (gpsiq_despread_kernels.hip, with gpsiq_despread_geometry.h) use of each other.  The plan is in
// gpsiq_despread_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `dsp`.
#ifndef GPSIQ_DESPREAD_H
#define GPSIQ_DESPREAD_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// the sums, satellites and stream statistics of one call on the device and page-locked on their way back, and the two events its
// kernel is timed with
struct DespreadSet {
    DevBuf<gpsiq_despread_sum_t>    d_sums;   PinnedBuf<gpsiq_despread_sum_t> h_sums;       // [nblocks][nchan][nseg]
    DevBuf<uint8_t>                 d_prn;    PinnedBuf<uint8_t>              h_prn;        // [nblocks][nchan]
    DevBuf<gpsiq_block_stats_t>     d_stats;  PinnedBuf<gpsiq_block_stats_t>  h_stats;      // [nblocks]
    Event          t0, t1;
    int            last[4] = {-1, 0, 0, 0};        // the last call's plan: kernel, slots, grid, wave_rows (gpsiq_despread_last_plan)
    int reserve(size_t nsums, size_t nprn, size_t nblocks);     // first use + room for one call
};

// (every pair grows together, device side first)
inline int DespreadSet::reserve(size_t nsums, size_t nprn, size_t nblocks)
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(reserve_together(nsums, nsums + nsums / 4 + 256, d_sums, h_sums));
    HIP_TRY(reserve_together(nprn, nprn + nprn / 4 + 256, d_prn, h_prn));
    HIP_TRY(reserve_together(nblocks, nblocks + nblocks / 4 + 16, d_stats, h_stats));
    return GPSIQ_OK;
}

// the correlator kernels (gpsiq_despread_kernels.hip): kernel and slots as gpsiq_despread_plan.h names them.  Arguments: descriptors,
// nchan, nsamp, src, block stride, block0, tables, workgroups per block, rows per wave, rows per segment, segments per block, clip,
// sums, satellites, stream statistics (may be null)
using DespreadFn  = void (*)(const gpsiq_qchan_t *, int, int, const uint8_t *, size_t, int, const DeviceTables *, int, int, int, int, int,
                             gpsiq_despread_sum_t *, uint8_t *, gpsiq_block_stats_t *);
DespreadFn  despread_kernel(int fmt, int kernel, int slots);

}  // namespace gpsiq

// gpsiq_despread.cpp: gpsiq_despread itself, behind the plumbing entry "despread".  Declared from the public prototype, and hidden:
// a definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_despread) gpsiq_despread_impl;
#endif
