// gpsiq_acquire_geometry.h -- the geometry the acquisition kernels (gpsiq_acquire_kernels.hip) are compiled for and the planner
// (gpsiq_acquire_plan.h) cuts its grids and sizes its scratch by.  These numbers decide device code, so the file is one of the device
// sources behind gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain C++: the planner compiles without HIP.
#ifndef GPSIQ_ACQUIRE_GEOMETRY_H
#define GPSIQ_ACQUIRE_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kAcqThreads = 256;               // generic, wipe and peak kernels: threads per workgroup
// the matrix path: one v_mfma_i32_16x16x64_i8 multiplies 16 rows x 64 samples by 64 samples x 16 shifts
constexpr int kAcqTileRows = 16;               // rows of a tile: 2 bins x (I, Q) x 4 digit rows (int8 fills 3 of every 4)
constexpr int kAcqBinsPerTile = 2;
constexpr int kAcqK = 64;                      // samples per k-step
constexpr int kAcqTileCols = 16;               // columns of a tile: shifts 16 apart, so that one residue serves all 16 lanes
constexpr int kAcqBlockShifts = 256;           // shifts one wave owns: 16 tiles, one per residue, against the same plane fragment
constexpr int kAcqWaves = 4;                   // waves of an acquire_mfma workgroup: four row tiles against one satellite's code copies
// the 16 zero-padded copies of the sampled code, one per residue, live in LDS: a unit of 16 zeros, ncoh + 16 bytes of (shifted) code,
// a unit of 16 zeros -- 16 * (ncoh + kAcqCopyPad) bytes within the 64 KiB a kernel takes without asking for more
constexpr int kAcqCopyPad = 48;
constexpr int kAcqMaxFastNcoh = 3072;
constexpr int kAcqPlaneTail = 320;             // plane bytes past the last sample a k-step can touch (4 extra k-steps + one fragment)
constexpr uint64_t kAcqScratchCap = UINT64_C(256) << 20;      // bytes of digit planes above which the planner takes the generic kernel

}  // namespace gpsiq
#endif
