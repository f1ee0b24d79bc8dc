// gpsiq_resample_geometry.h -- the geometry the resampler kernels (gpsiq_resample_kernels.hip) are compiled for and the planner
// (gpsiq_resample_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants: host and device code include it alike.
#ifndef GPSIQ_RESAMPLE_GEOMETRY_H
#define GPSIQ_RESAMPLE_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kRsThreads = 256;                // four waves per workgroup, both kernels
constexpr int kRsMaxTaps = 64, kRsMaxLog2Phases = 8, kRsMaxShift = 16;
constexpr int kRsMaxTable = 8256;              // (nphases + 1) * ntaps at most: 129 rows of 64 taps, 257 rows of 32
constexpr long kRsTapSum = 65535;              // sum |taps[r][k]| of a row at most: |a0|, |a1| <= 65535 * 32768 < 2^31
constexpr uint64_t kRsMinStep = UINT64_C(1) << 29, kRsMaxStep = UINT64_C(1) << 35, kRsOne = UINT64_C(1) << 32;   // 2^-32 input sample
constexpr unsigned kRsMaxGrid = 1024;          // workgroups of a launch at most: each stages the tap table once and strides over its units

// The tap table in LDS, both kernels: row r is ntaps int16 taps packed two to a dword (tap 2c below, 2c + 1 above, a missing one
// zero) at dword r * resample_tap_stride(ntaps).  The stride is ODD, so that lanes whose phases differ read different banks at the
// same tap (ds_read_b32 banks are dword mod 32); lanes of one phase read one address, which is a broadcast.
constexpr int resample_tap_stride(int ntaps) { return ((ntaps + 1) / 2) | 1; }
constexpr int resample_table_dwords(int log2_phases, int ntaps) { return ((1 << log2_phases) + 1) * resample_tap_stride(ntaps); }

// resample_rows: a RUN is the kRsRun consecutive outputs a workgroup makes from one staged window, one dword per input sample (I
// below, Q above, sign-extended to 16 bits).  The window of a run of n outputs starts at x(m_first - (ntaps - 1)) and ends at x(m_last):
// ((n - 1) * step >> 32) + 1 + ntaps samples at the most.
constexpr int kRsRun = 512;
constexpr int resample_window(int n, uint64_t step, int ntaps) { return (int) (((uint64_t) (n - 1) * step) >> 32) + 1 + ntaps; }
// From this step on (two input samples per output) neighbouring lanes read the window two or more dwords apart, up to eight: 32
// lanes then meet on 32 / stride banks.  The PAD variant of the kernel keeps sample i of the window at dword i + (i >> 5): at a
// stride of eight, lanes 4g .. 4g + 3 read banks g, g + 8, g + 16, g + 24 -- all 32 different.  Below it the plain layout stays: lanes
// read neighbouring dwords, and the index arithmetic of the padding would be paid for nothing.
constexpr uint64_t kRsPadStep = UINT64_C(1) << 33;
constexpr int resample_window_dwords(int window, bool pad) { return pad ? window + (window >> 5) + 1 : window; }

// resample_generic: one output per thread, kRsThreads outputs per unit, samples from global memory
constexpr int kRsGenericUnit = kRsThreads;

}  // namespace gpsiq
#endif
