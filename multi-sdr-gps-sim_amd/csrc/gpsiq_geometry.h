// gpsiq_geometry.h -- the workgroup geometry the synthesis kernels (gpsiq_kernels.hip) are compiled for and the launch planner
// (gpsiq_launch_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile); the planner and the launcher are not.  Plain C++: the planner compiles without HIP.
#ifndef GPSIQ_GEOMETRY_H
#define GPSIQ_GEOMETRY_H

namespace gpsiq {

// generic kernel: one sample per thread per step
constexpr int kGenericThreads = 256;

// row kernels: a "row" is 64 consecutive samples, one per lane of a wave; each wave of synth_rows / synth_rowsx owns
// kRowsPerWave consecutive rows
constexpr int kWaves = 8;
constexpr int kRowsPerWave = 32;
constexpr int kRowsThreads = kWaves * 64;
constexpr int kRowsTile = kWaves * kRowsPerWave * 64;   // 16384 samples

// segm's pre-pass (sign_masks)
constexpr int kMaskRowsPerThread = 16;      // consecutive rows one pre-pass thread walks (one division per 1024 samples)
constexpr int kMaskThreads = 256;

// segb, rows per chunk: the lane groups of the window builder need 4 windows each.
// 4 KB of LUT per channel: with 16 channels two 8-wave workgroups still fit a CU (the same four waves per SIMD as
// seg) when a chunk is 16 rows, i.e. 8 KB of windows per workgroup (64 + 8 + 3 KB, twice = 150 of 160 KB); a single
// 16-wave workgroup per CU with 64-row chunks measured 10 % SLOWER than seg although its waves ran 11 % faster
// (SQ_WAVE_CYCLES): with one workgroup per CU nothing fills the CU while that workgroup starts up or drains.
constexpr int both_rows(int slots) { return slots == 4 ? 64 : slots == 8 ? 32 : 16; }

}  // namespace gpsiq
#endif
