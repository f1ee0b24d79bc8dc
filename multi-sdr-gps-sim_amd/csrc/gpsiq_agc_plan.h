// gpsiq_agc_plan.h -- what a gpsiq_agc call or a piece of gpsiq_generate_batch_agc (include/gpsiq_rows.h, "AGC") takes: the windows
// a span touches, the grids of the three launches and the scratch they share.  Host code only, and pure: no HIP, no environment.  The
// piece size of the batch call is stage_piece_blocks (gpsiq_pieces.h), with the GPSIQ_AGC_PIECE_BLOCKS override as an argument, read
// per call by the caller.  tests/agc_plan.cpp answers it for the tests.  Not a device source: the geometry the kernels are compiled
// for is gpsiq_agc_geometry.h, the list of kernels that exist is in gpsiq_agc_kernels.hip.
#ifndef GPSIQ_AGC_PLAN_H
#define GPSIQ_AGC_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_agc_geometry.h"
#include "gpsiq_pieces.h"

namespace gpsiq {

// windows a span of nsamp samples touches when `fill` samples of the window in progress lie before it, and the fill it leaves
inline void agc_span(uint64_t nsamp, uint32_t window, uint32_t fill, uint64_t *nwin, uint32_t *next_fill)
{
    const uint64_t end = (uint64_t) fill + nsamp;
    *nwin = nsamp ? (end + window - 1) / window : 0;
    *next_fill = (uint32_t) (end % window);
}

struct AgcPlan {
    bool     launch = false;           // false: no sample, nothing is launched
    bool     mask = false;             // the blanker is on: agc_measure writes a bit per sample, agc_apply reads it
    unsigned threads = 0;
    unsigned measure_grid = 0;         // one workgroup per tile of kAgcTile samples
    unsigned gains_grid = 0;           // one thread per touched window
    unsigned apply_grid = 0;           // one workgroup per kAgcApplyTile samples
    uint32_t units = 0;                // units of the span (gpsiq_agc_geometry.h), the last one possibly ragged
    uint64_t nwin = 0;                 // windows touched
    uint32_t next_fill = 0;
    // the scratch, in bytes from its start: per window the sum (uint64) at 0, the count (uint32) at off_cnt -- zeroed per launch,
    // zero_bytes from 0 --, the multiplier (uint32) at off_mult; the mask, a byte per unit, at off_mask (only where mask)
    size_t   off_cnt = 0, off_mult = 0, off_mask = 0, zero_bytes = 0, scratch_bytes = 0;
};

inline AgcPlan plan_agc(int nsamp, int window, uint32_t fill, bool mask)
{
    AgcPlan p;
    p.mask = mask;
    if (nsamp <= 0 || window < kAgcMinWindow || window > kAgcMaxWindow || fill >= (uint32_t) window) return p;
    agc_span((uint64_t) nsamp, (uint32_t) window, fill, &p.nwin, &p.next_fill);
    p.launch = true;
    p.threads = kAgcThreads;
    p.units = (uint32_t) (((uint64_t) nsamp + kAgcUnit - 1) / kAgcUnit);
    p.measure_grid = (unsigned) (((uint64_t) nsamp + kAgcTile - 1) / kAgcTile);
    p.gains_grid = (unsigned) ((p.nwin + kAgcThreads - 1) / kAgcThreads);
    p.apply_grid = (unsigned) (((uint64_t) nsamp + kAgcApplyTile - 1) / kAgcApplyTile);
    const size_t up = 15;
    p.off_cnt = (8 * (size_t) p.nwin + up) & ~up;
    p.zero_bytes = p.off_cnt + 4 * (size_t) p.nwin;
    p.off_mult = (p.zero_bytes + up) & ~up;
    p.off_mask = (p.off_mult + 4 * (size_t) p.nwin + up) & ~up;
    p.scratch_bytes = p.off_mask + (mask ? (size_t) p.units : 0);
    return p;
}

// Blocks per piece of gpsiq_generate_batch_agc: the one policy, stage_piece_blocks (gpsiq_pieces.h), under the call's name.  A piece
// is one span of the stage: its samples fit an int
inline int agc_piece_blocks(int nblocks, int nsamp, size_t src_block_bytes, long override_blocks) { return stage_piece_blocks(nblocks, nsamp, src_block_bytes, override_blocks); }

}  // namespace gpsiq
#endif
