// gpsiq_filter_geometry.h -- the geometry the filter kernels (gpsiq_filter_kernels.hip) are compiled for and the planner
// (gpsiq_filter_plan.h) cuts its grids by.  These numbers decide device code, so the file is one of the device sources behind
// gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants: host and device code include it alike.
#ifndef GPSIQ_FILTER_GEOMETRY_H
#define GPSIQ_FILTER_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kFiltThreads = 256;              // four waves per workgroup, both kernels
constexpr int kFiltMaxTaps = 512, kFiltMaxDecim = 16, kFiltMaxShift = 24;
constexpr unsigned kFiltMaxGrid = 1u << 20;    // workgroups of a launch at most; the kernels stride over runs past that
constexpr long kFiltTapSum = 65535;            // sum |taps[k]| at most: |acc| <= 65535 * 32768 < 2^31

// A RUN is the outputs one workgroup makes from one staged window: a multiple of kFiltThreads outputs, kFiltMaxRun at the most.
// The window of a run of n outputs is (n - 1) * decim + ntaps input samples.
constexpr int kFiltMaxRun = 1024;
// filter_generic keeps the window as one dword per sample (I below, Q above, sign-extended to 16 bits) and the taps as dwords behind it
constexpr int kFiltGenericWindow = 8192;       // samples; 255 * 16 + 512 = 4592 fit: a run is never below kFiltThreads outputs
constexpr int filter_generic_run(int ntaps, int decim)
{
    const int fit = (kFiltGenericWindow - ntaps) / decim + 1;
    return fit >= kFiltMaxRun ? kFiltMaxRun : fit / kFiltThreads * kFiltThreads;
}

// filter_mfma (int8 input): v_mfma_i32_16x16x64_i8, D = A x B.  The stream is one real sequence of bytes X[e], e = 2 m + c (c = 0: I,
// 1: Q), the taps zero-stuffed T[2 k] = taps[k].  A TILE is 16 rows x 16 columns: column col is 8 consecutive outputs, row r = 2 jj + c
// their component c of output jj; the k dimension runs over the bytes of the column's window from its first byte on, 64 per step.
//   A(r, k) = T[2 jj decim + c + 2 (ntaps - 1) - k]   (0 outside the taps and at odd arguments): the same for every column and tile
//   B(k, col) = X[first byte of the column's window + k]
// A wave does whole tiles of 128 outputs; kFiltMfmaSteps(ntaps, decim) k-steps cover 14 decim + 2 ntaps bytes.
constexpr int kFiltTileOutputs = 128, kFiltColOutputs = 8, kFiltK = 64;
constexpr int filter_mfma_steps(int ntaps, int decim) { return (14 * decim + 2 * ntaps + kFiltK - 1) / kFiltK; }
// two digit planes of kFiltK * 16 bytes per k-step, in fragment order: lane l's 16 bytes of (plane p, step t) at ((p * steps + t) * 64 + l) * 16
constexpr int filter_mfma_plane_bytes(int steps) { return 2 * steps * kFiltK * 16; }
constexpr int kFiltMaxSteps = filter_mfma_steps(kFiltMaxTaps, kFiltMaxDecim);          // 20
// the staged bytes of a run of `run` outputs: every column's k range, zeros past the span
constexpr int filter_mfma_window_bytes(int run, int decim, int steps) { return 2 * decim * (run - kFiltColOutputs) + kFiltK * steps; }
constexpr int kFiltMfmaLds = 65536 - 64;       // planes + window at most (the workgroup's partial counts lie beside them)
constexpr int filter_mfma_run(int ntaps, int decim)
{
    const int steps = filter_mfma_steps(ntaps, decim);
    return filter_mfma_plane_bytes(steps) + filter_mfma_window_bytes(kFiltMaxRun, decim, steps) <= kFiltMfmaLds ? kFiltMaxRun : kFiltMaxRun / 2;
}
// a tap splits into two signed bytes, taps[k] = d0 + 256 d1 with d0 in [-128, 127]: d1 fits a signed byte up to this tap
constexpr int kFiltMfmaMaxTap = 127 * 256 + 127;

}  // namespace gpsiq
#endif
