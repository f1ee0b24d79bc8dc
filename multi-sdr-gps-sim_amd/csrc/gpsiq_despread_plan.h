// gpsiq_despread_plan.h -- which correlator kernel a gpsiq_despread call (include/gpsiq_rows.h, "Despread") takes, and with which
// grid.  Host code only, and pure: no HIP, no environment (every knob is an argument).  tests/despread_plan.cpp pins every plan on
// the CPU.  Not a device source: the geometry the kernels are compiled for is gpsiq_despread_geometry.h, the list of kernels that
// exist is in gpsiq_despread_kernels.hip.
#ifndef GPSIQ_DESPREAD_PLAN_H
#define GPSIQ_DESPREAD_PLAN_H

#include <cstdint>

#include "gpsiq_despread_geometry.h"
#include "gpsiq_launch_plan.h"

namespace gpsiq {

enum DespreadKernel { kDespreadGeneric = 0, kDespreadRows = 1 };

inline const char *despread_kernel_name(int k) { return k == kDespreadRows ? "rows" : "generic"; }

struct DespreadPlan {
    int      kind = kPlanNothing;      // kPlanNothing: no block to work on (nothing is launched) | kPlanLaunch
    int      kernel = kDespreadGeneric;
    int      slots = 0;                // rows: channel slots the kernel is unrolled for (4, 8, 12, 16); generic: 0
    unsigned grid = 0, threads = 0;
    int      tiles = 0;                // workgroups per block
    int      wave_rows = 0;            // consecutive rows (64 samples each) one wave owns
    int      seg_rows = 0;             // rows per segment (seg_len / 64)
    int      nseg = 0;                 // segments per block
};

// segments of a block: ceil(nsamp / seg_len)
inline int despread_nseg(int nsamp, int seg_len) { return nsamp <= 0 || seg_len <= 0 ? 0 : (int) (((int64_t) nsamp + seg_len - 1) / seg_len); }

// force_generic: the caller asks for the fallback where the row kernel would do (the cross-check of the tests); the reverse does not
// exist -- a set the row kernel cannot serve always takes the generic one.
// The row kernel serves what the default `seg` synthesis serves: every lane of a row inside one 32-chip window (kRowsMaxCodeStep).
// A wave owns wave_rows consecutive rows of one block; kDespreadWaves waves make a workgroup.  Long runs amortise the per-workgroup
// set-up (table, codes) and cut the number of atomics, short ones fill the device: the run is halved from kDespreadMaxWaveRows down
// to one chunk while the grid has fewer than target_wgs workgroups (kDespreadTargetWgs; GPSIQ_DESPREAD_TARGET_WGS in the environment
// of the caller, for experiments and for tests that want long runs on short streams).  The generic kernel has fixed runs.
inline DespreadPlan plan_despread(int nsamp, int nblocks, int seg_len, const SynthClass &cls, bool force_generic,
                                  int target_wgs = kDespreadTargetWgs)
{
    DespreadPlan p;
    if (nblocks <= 0 || nsamp < 0 || seg_len < 64 || (seg_len & 63)) return p;
    p.kind = kPlanLaunch;
    p.kernel = !force_generic && cls.max_code_step <= kRowsMaxCodeStep ? kDespreadRows : kDespreadGeneric;
    p.threads = kDespreadWaves * 64;
    p.seg_rows = seg_len / 64;
    p.nseg = despread_nseg(nsamp, seg_len);
    const int rows_total = (int) (((int64_t) nsamp + 63) / 64);      // (no int overflow next to INT_MAX)
    if (p.kernel == kDespreadRows) {
        p.slots = cls.max_active <= 4 ? 4 : cls.max_active <= 8 ? 8 : cls.max_active <= 12 ? 12 : 16;
        p.wave_rows = kDespreadMaxWaveRows;
        auto tiles_of = [&](int wr) { return (rows_total + kDespreadWaves * wr - 1) / (kDespreadWaves * wr); };
        while (p.wave_rows > kDespreadChunkRows && (int64_t) tiles_of(p.wave_rows) * nblocks < target_wgs) p.wave_rows /= 2;
        p.tiles = tiles_of(p.wave_rows);
    } else {
        p.wave_rows = kDespreadGenericWaveRows;
        p.tiles = (rows_total + kDespreadWaves * p.wave_rows - 1) / (kDespreadWaves * p.wave_rows);
    }
    if (p.tiles < 1) p.tiles = 1;      // a block of no samples still reports its satellites
    p.grid = (unsigned) p.tiles * (unsigned) nblocks;
    return p;
}

}  // namespace gpsiq
#endif
