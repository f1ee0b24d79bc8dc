// gpsiq_despread_geometry.h -- the workgroup geometry the correlator kernels (gpsiq_despread_kernels.hip) are compiled for and the
// planner (gpsiq_despread_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources
// behind gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain C++: the planner compiles without HIP.
#ifndef GPSIQ_DESPREAD_GEOMETRY_H
#define GPSIQ_DESPREAD_GEOMETRY_H

namespace gpsiq {

constexpr int kDespreadWaves = 4;              // waves per workgroup, both kernels
// row kernel: a wave builds the sign windows of kDespreadChunkRows rows at a time and widens its 32-bit per-lane partial sums at
// the end of every chunk at the latest: 64 rows x 2 * 32768 * 250 = 1 048 576 000 < 2^31
constexpr int kDespreadChunkRows = 64;
constexpr int kDespreadMaxWaveRows = 256;      // longest run of rows a wave owns
constexpr int kDespreadTargetWgs = 2048;       // the planner shortens the runs while the grid is smaller than this
// generic kernel: a wave owns 16 consecutive rows (a workgroup 4096 samples, as synth_generic's tile)
constexpr int kDespreadGenericWaveRows = 16;

}  // namespace gpsiq
#endif
