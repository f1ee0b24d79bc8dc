// gpsiq_resample_plan.h -- the output count, the kernel and the grid a gpsiq_resample call (include/gpsiq_rows.h, "Resample") takes,
// and the staging a piece of gpsiq_generate_batch_resampled asks for.  Host code only, and pure: no HIP, no environment (the
// GPSIQ_RESAMPLE_KERNEL override is an argument, read per call by the caller; so is GPSIQ_RESAMPLE_PIECE_BLOCKS, for the piece size
// of the batch call: stage_piece_blocks, gpsiq_pieces.h).  tests/resample_plan.cpp pins every plan on the CPU.  Not a device
// source: the geometry the kernels are compiled for is gpsiq_resample_geometry.h.
#ifndef GPSIQ_RESAMPLE_PLAN_H
#define GPSIQ_RESAMPLE_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_resample_geometry.h"
#include "gpsiq_pieces.h"

namespace gpsiq {

constexpr uint64_t kRsMaxSpan = UINT64_C(1) << 60;       // nsamp of gpsiq_resample_span below this: eight outputs a sample fit 64 bits
constexpr uint64_t kRsMaxPos = UINT64_C(1) << 63;        // pos0 below this

// outputs of a span and the position its continuation starts at (include/gpsiq_rows.h: gpsiq_resample_span); arguments in range.
// nsamp * 2^32 passes 64 bits from nsamp = 2^32 on: the end of the span is a 128-bit number
inline void resample_span(uint64_t nsamp, uint64_t pos0, uint64_t step, uint64_t *nout, uint64_t *next_pos)
{
    const unsigned __int128 end = (unsigned __int128) nsamp << 32;
    const unsigned __int128 n = (unsigned __int128) pos0 >= end ? 0 : (end - pos0 + (step - 1)) / step;
    *nout = (uint64_t) n;
    *next_pos = (uint64_t) ((unsigned __int128) pos0 + n * step - end);
}

enum { kRsGeneric = 0, kRsRows = 1 };
enum { kRsAuto = 0, kRsForceGeneric = 1, kRsForceRows = 2 };

// Both kernels serve every legal call.  The row kernel is the default.  profiles/resample_rates.txt (MI355X, 26e6 input samples,
// designed taps): it is the faster of the two at every measured row -- 0.35 to 0.38 of the generic kernel's time at 2.6 to 2.048 Msps
// and at a 20 ppm offset (int8 and int16, 128 phases of 16 taps, with and without interp), 0.35 eight up, 0.29 at 64 phases of 64
// taps, 0.91 eight down -- so no shape is sent to resample_generic.
constexpr int kRsDefaultKernel = kRsRows;

struct ResamplePlan {
    bool     launch = false;           // false: no output, nothing is launched
    int      kernel = kRsGeneric;
    uint64_t nout = 0, next_pos = 0;
    unsigned grid = 0, threads = 0;
    int      run = 0;                  // outputs of a unit: a run of resample_rows, a workgroup's threads for resample_generic
    bool     pad = false;              // resample_rows: the padded window (gpsiq_resample_geometry.h)
    uint64_t runs = 0;                 // units of the launch: workgroup w takes units w, w + grid, ...
    size_t   lds = 0;                  // dynamic LDS of the launch, bytes
};

// arguments in range (the caller has checked them); force: kRsAuto, or the kernel GPSIQ_RESAMPLE_KERNEL names
inline ResamplePlan plan_resample(uint64_t nsamp, int log2_phases, int ntaps, uint64_t step, uint64_t pos0, int force)
{
    ResamplePlan p;
    resample_span(nsamp, pos0, step, &p.nout, &p.next_pos);
    if (p.nout == 0) return p;
    p.launch = true;
    p.threads = kRsThreads;
    p.kernel = force == kRsForceGeneric ? kRsGeneric : force == kRsForceRows ? kRsRows : kRsDefaultKernel;
    const size_t table = 4 * (size_t) resample_table_dwords(log2_phases, ntaps);
    if (p.kernel == kRsRows) {
        p.run = kRsRun;
        p.pad = step >= kRsPadStep;
        p.lds = table + 4 * (size_t) resample_window_dwords(resample_window(kRsRun, step, ntaps), p.pad);
    } else {
        p.run = kRsGenericUnit;
        p.lds = table;
    }
    p.runs = (p.nout + (uint64_t) p.run - 1) / (uint64_t) p.run;
    p.grid = p.runs < kRsMaxGrid ? (unsigned) p.runs : kRsMaxGrid;
    return p;
}

// Blocks per piece of gpsiq_generate_batch_resampled: the one policy, stage_piece_blocks (gpsiq_pieces.h), under the call's name.  A
// piece is one span of the resampler: its samples fit an int
inline int resample_piece_blocks(int nblocks, int nsamp, size_t src_block_bytes, long override_blocks) { return stage_piece_blocks(nblocks, nsamp, src_block_bytes, override_blocks); }

// the outputs a piece of `samples` input samples can give at the most, whatever its pos0: what the batch call sizes its staging by
inline uint64_t resample_piece_outputs(uint64_t samples, uint64_t step) { return (uint64_t) ((((unsigned __int128) samples << 32) + step - 1) / step); }

}  // namespace gpsiq
#endif
