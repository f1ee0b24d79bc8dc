// gpsiq_stap_beams_geometry.h -- the constants the kernels of gpsiq_stap_beams (gpsiq_stap_beams_kernels.hip) are compiled for and the
// host plans with (gpsiq_stap_beams_plan.h): the operands of the matrix kernel, the k-byte order, the tile, the chunk, the plane bounds.
// A device source (behind gpsiq_kernels_id()); no HIP in it, so tests/stap_beams_plan.cpp includes it with the host compiler.
//
// The product.  y_b(n) = sum over e, t of w_b[e][t] x_e(n - t) for up to eight beams b is D = A B of v_mfma_i32_16x16x64_i8:
//   A [16][64]   row 2 b is the real component of beam b, row 2 b + 1 its imaginary one; rows of absent beams are zero
//   B [64][16]   column c is the space-time snapshot of one sample, 64 k-bytes: 32 complex rows at most
//   D [16][16]   D(2 b, c) = accI and D(2 b + 1, c) = accQ of beam b at column c's sample
// The k-bytes.  An element's taps are padded to TP = 1, 2, 4 or 8 (beams_padded_taps; the padding's weights are zero), so that the
// window x_e(n - TP + 1 .. n) of a sample is 2 TP consecutive bytes of an int8 stream and a lane's 16 k-bytes are 8 / TP whole windows:
//   k = 2 TP e + 2 (TP - 1 - t) + c        element e, tap t, component c (0: I, 1: Q) -- the bytes as they lie in memory
// and A is built to match: row 2 b holds re at the byte of I and -im at the byte of Q, row 2 b + 1 holds im and re there.  K' = E TP
// must not pass 32; a shape whose padding would (5 x 5, 4 x 5 fits: 32) goes to the generic kernel.
// Lanes (gpsiq_acquire_kernels.hip measured the map): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds column
// l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2): lane (col, g) ends with beams 2 g and 2 g + 1,
// both components, of column col.
#ifndef GPSIQ_STAP_BEAMS_GEOMETRY_H
#define GPSIQ_STAP_BEAMS_GEOMETRY_H

#include <cstdint>

#include "gpsiq_filter_geometry.h"
#include "gpsiq_stap_geometry.h"

namespace gpsiq {

constexpr int kBeamsMax = 8;                         // GPSIQ_STAP_MAX_BEAMS (include/gpsiq_rows.h; gpsiq_stap_beams.h asserts it)
constexpr int kBeamsThreads = 256, kBeamsWaves = kBeamsThreads / 64;
constexpr int kBeamsRows = 16, kBeamsCols = 16, kBeamsK = 64;         // the instruction's M, N, K
constexpr int kBeamsPlaneBytes = kBeamsRows * kBeamsK;                // one digit plane of A in fragment order: lane l's 16 bytes at 16 l
static_assert(2 * kBeamsMax == kBeamsRows && 2 * kStapMaxRows == kBeamsK, "eight beams fill the rows of A, 32 complex rows its k-bytes");

// the padded taps of an element, 0 where the matrix kernel cannot serve the shape: the next power of two, while K' = nelem * TP fits
constexpr int beams_padded_taps(int nelem, int ntaps)
{
    const int tp = ntaps <= 1 ? 1 : ntaps <= 2 ? 2 : ntaps <= 4 ? 4 : 8;
    return nelem * tp <= kStapMaxRows ? tp : 0;
}
constexpr int beams_kbyte(int tp, int e, int t, int c) { return 2 * tp * e + 2 * (tp - 1 - t) + c; }

// A lane ends with S consecutive samples of two beams, 16 bytes of each beam's stream: column col of step j is sample S col + j of the
// wave's tile.  A wave's tile is 16 S samples, a workgroup's chunk four of them: what is staged in LDS at a time, and a workgroup's run.
constexpr int beams_lane_samples(int out_size) { return 16 / (2 * out_size); }            // S: 8 (int8 out), 4 (int16 out)
constexpr int beams_tile_samples(int out_size) { return kBeamsCols * beams_lane_samples(out_size); }
constexpr int beams_chunk_samples(int out_size) { return kBeamsWaves * beams_tile_samples(out_size); }
constexpr unsigned kBeamsMaxGrid = 2048;             // workgroups take the chunks b, b + grid, ...
// An element's staged row: the samples c0 - H .. c0 + chunk - 1 of a chunk that starts at c0, H = TP (0 at TP = 1: nothing before the
// sample itself is read), as dwords of two samples -- c0 - H is even, so a dword of the row is an aligned dword of an int8 stream --
// and one dword more: a window that starts at an odd sample is taken from one dword more by a 16-bit funnel shift.
constexpr int beams_stage_back(int tp) { return tp == 1 ? 0 : tp; }
constexpr int beams_row_dwords(int out_size, int tp) { return (beams_chunk_samples(out_size) + beams_stage_back(tp)) / 2 + 1; }
constexpr int beams_max_elem(int tp) { return kStapMaxRows / tp < kStapMaxElem ? kStapMaxRows / tp : kStapMaxElem; }
// the dwords of a row a lane loads for its S windows of one element: they overlap, S + TP samples in all from an even sample on
constexpr int beams_lane_dwords(int out_size, int tp) { return beams_lane_samples(out_size) / 2 + tp / 2 + 1; }
static_assert((beams_chunk_samples(1) - beams_lane_samples(1)) / 2 + beams_lane_dwords(1, 8) <= beams_row_dwords(1, 8) &&
              (beams_chunk_samples(2) - beams_lane_samples(2)) / 2 + beams_lane_dwords(2, 8) <= beams_row_dwords(2, 8) &&
              (beams_chunk_samples(1) - beams_lane_samples(1)) / 2 + beams_lane_dwords(1, 1) <= beams_row_dwords(1, 1) &&
              (beams_chunk_samples(2) - beams_lane_samples(2)) / 2 + beams_lane_dwords(2, 2) <= beams_row_dwords(2, 2),
              "the last lane of a chunk reads inside its staged row");
static_assert(4 * 2 * kStapMaxElem * beams_row_dwords(1, 4) <= 65536, "two byte planes of eight elements fit the LDS of a workgroup");

// The planes.  An entry of A (re, +im, -im of an int16 weight) goes in as two balanced digits, entry = d0 + 256 d1, both signed bytes:
// gpsiq_filter's restriction, entries up to kFiltMfmaMaxTap (32639; -32768 splits).  A row holds at most 64 entries whose magnitudes
// sum to at most 65535 (the call's bound, per beam): sum |d0| <= 64 * 128 = 2^13 and sum |d1| <= 65535 / 256 + 64 < 2^9.
//   int8 input:   P0 = d0 . x, P1 = d1 . x with |x| <= 128: |P0| <= 2^20, |P1| < 2^16; acc = P0 + 256 P1.
//   int16 input:  x = 256 hi + lo' + 128 (lo' = (x & 255) - 128, hi = x >> 8, both signed bytes), so
//                 acc = P00 + 256 (P01 + P10) + 65536 P11 + 128 sum of the row's entries,   Pij = d_i . (lo' | hi)_j,
//                 every P inside 2^20 and P01 + P10 inside 2^21.  A sample the contract calls zero is the pair (lo' = -128, hi = 0).
// The sums are NOT term by term inside int32 (65536 P11 can pass 2^32), but their value is acc and |acc| <= 65535 * 32768 < 2^31: added
// in uint32, modulo 2^32, and read back as int32 they are exact.
constexpr int kBeamsMaxEntry = kFiltMfmaMaxTap;
static_assert((int64_t) kBeamsK * 128 * 128 <= (int64_t) 1 << 20, "a plane product of 64 k-bytes is inside 2^20");
static_assert((int64_t) kStapWeightSum * 32768 < (int64_t) 1 << 31, "the sum itself is inside int32: the recombination modulo 2^32 is exact");
static_assert(kBeamsMaxEntry == 127 * 256 + 127, "two balanced digits hold -32896 .. 32639");

// What the host sends ahead of a launch, as dwords: the two planes, the 16 row constants 128 sum_k A(row, k) (int16 input), and the
// weights [kBeamsMax][kStapMaxRows] as stap_combine has them (re low, im high) for the generic kernel.
constexpr int kBeamsConstAt = 2 * kBeamsPlaneBytes / 4;
constexpr int kBeamsWeightsAt = kBeamsConstAt + kBeamsRows;
constexpr int kBeamsCoefDwords = kBeamsWeightsAt + kBeamsMax * kStapMaxRows;

// ---- stap_beams_generic --------------------------------------------------------------------------------------------------------------
// stap_combine's scheme, a loop over the beams around it: a lane owns a slot of S samples from sample S u on (no lead: the destinations
// of one call are aligned each in its own way, so a full slot is stored as 16 bytes where its address allows and as four dwords else).
constexpr unsigned kBeamsGenMaxGrid = 8192;

}  // namespace gpsiq
#endif
