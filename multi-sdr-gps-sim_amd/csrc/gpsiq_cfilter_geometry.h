// gpsiq_cfilter_geometry.h -- the geometry the complex filter's kernels (gpsiq_cfilter_kernels.hip) are compiled for and its planner
// (gpsiq_cfilter_plan.h) cuts its grids by.  The stage keeps gpsiq_filter's contract, so runs, tiles, k-steps, plane order and limits
// are those of gpsiq_filter_geometry.h; what is written here is what complex taps and an int16 stream add.  These numbers decide device
// code, so the file is one of the device sources behind gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants: host and
// device code include it alike.
#ifndef GPSIQ_CFILTER_GEOMETRY_H
#define GPSIQ_CFILTER_GEOMETRY_H

#include <cstdint>

#include "gpsiq_filter_geometry.h"

namespace gpsiq {

// sum (|re[k]| + |im[k]|) at most: |accI|, |accQ| <= 65535 * 32768 = 2^31 - 32768 < 2^31 for both input formats
constexpr long kCfiltTapSum = kFiltTapSum;

// cfilter_generic keeps the window as filter_generic does (one dword per sample) and the taps behind it as one dword per tap, re in
// the low half and im in the high half: the same LDS bytes, so filter_generic_run() is the run.

// The matrix operand of complex taps.  filter_mfma's stream is one real byte sequence X[2 m + c] and its A(r, k) is zero at every odd
// argument of the zero-stuffed taps.  With h = re + j im those odd arguments hold the cross terms: for row r = 2 jj + c and tap k, with
// k_I = 2 jj decim + 2 (ntaps - 1) - 2 k the byte at which the row's window holds I(m_j - k) and k_Q = k_I + 1 the one of Q(m_j - k),
//   row (jj, 0) meets  re[k] at k_I and -im[k] at k_I + 1        accI = sum re I - im Q
//   row (jj, 1) meets  re[k] at k_Q and +im[k] at k_Q - 1        accQ = sum re Q + im I
// The largest k a row meets is 14 decim + 2 (ntaps - 1) + 1 (jj = 7, tap 0: row c = 0 at k_I + 1, row c = 1 at k_Q, the same byte) and
// the smallest is 0 (jj = 0, tap ntaps - 1): the k range of a tile is the real filter's, [0, 14 decim + 2 ntaps), and
// filter_mfma_steps(), filter_mfma_plane_bytes() and filter_mfma_window_bytes() hold unchanged (tests/cfilter_plan.cpp multiplies it out).
// Digit planes of 2 ntaps entries a row: entry = d0 + 256 d1 as in filter_mfma; sum |d0| <= 128 * 1024 and bytes of magnitude <= 128
// give |P0| <= 128 * 128 * 1024 = 2^24; |d1| <= (|entry| + 128) / 256, so sum |d1| <= (65535 + 128 * 1024) / 256 < 768, |P1| < 768 * 128
// < 2^17 and |256 P1| < 2^25: filter_mfma's int32 recombination P0 + 256 P1 holds for these planes as it stands.
// An entry splits into two signed bytes up to kFiltMfmaMaxTap; the entries are re, +im and -im, so the matrix kernels serve where
// max re <= 32639 and max |im| <= 32639 (im = -32768 would need -im = 32768).

// cfilter_mfma16 (int16 input): the window of a run as TWO byte planes, each laid out like filter_mfma's int8 window,
//   x = 256 hi + lo' + 128,   hi = x >> 8 (arithmetic) in [-128, 127],   lo' = (x & 255) - 128 in [-128, 127]
// exact for every int16 x.  A sample the contract calls zero is the pair (lo' = -128, hi = 0).  With A = d0 + 256 d1,
//   acc = P00 + 256 (P01 + P10) + 65536 P11 + 128 sum_k A(row, k),   Pab = sum_k da(row, k) * {lo', hi}b(k)
// and the last term depends on the row's component alone: 128 sum (re - im) for c = 0, 128 sum (re + im) for c = 1 (the host works
// both out once per call, cfilter_row_consts in gpsiq_cfilter_plan.h).
// LDS of a run: the two digit planes, then the lo' window, then the hi window, each window filter_mfma_window_bytes() long.
constexpr int cfilter_mfma16_lds(int run, int decim, int steps) { return filter_mfma_plane_bytes(steps) + 2 * filter_mfma_window_bytes(run, decim, steps); }
// the run shrinks 1024, 512, 256 until planes and windows fit kFiltMfmaLds; 0: nothing fits, the generic kernel serves
constexpr int kCfiltMinRun16 = 256;
constexpr int cfilter_mfma16_run(int ntaps, int decim)
{
    const int steps = filter_mfma_steps(ntaps, decim);
    for (int run = kFiltMaxRun; run >= kCfiltMinRun16; run /= 2)
        if (cfilter_mfma16_lds(run, decim, steps) <= kFiltMfmaLds) return run;
    return 0;
}
// (the largest legal shape, 512 taps at decim 16, fits at 256 outputs: 40960 + 2 * 9216 = 59392 bytes.  Inside the contract's ranges
// the fall to the generic kernel for want of LDS is therefore never taken; the planner keeps it for a geometry that changes.)
static_assert(cfilter_mfma16_run(kFiltMaxTaps, kFiltMaxDecim) == kCfiltMinRun16, "the int16 matrix path no longer fits its smallest run");

}  // namespace gpsiq
#endif
