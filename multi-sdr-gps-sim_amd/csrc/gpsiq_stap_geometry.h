// gpsiq_stap_geometry.h -- the constants the kernels of gpsiq_stap_cov / gpsiq_stap_combine (gpsiq_stap_kernels.hip) are compiled for
// and the host plans with (gpsiq_stap_plan.h): the rows, the Gram tiles of the matrix kernel, the runs, the flush bound, the slot of the
// combiner.  A device source (behind gpsiq_kernels_id()); no HIP in it, so tests/stap_plan.cpp includes it with the host compiler.
//
// The rows.  Row k = e T + t of the space-time snapshot is z_k(n) = x_e(n - t), K = E T <= 32 of them.  Its two components are the REAL
// rows 2 k + c, 2 K <= 64 of them, taken in G = ceil(K / 8) groups of 16: group g holds real rows 16 g .. 16 g + 15, rows from 2 K on
// all zero.  The Gram matrix  Gm[i][j] = sum over n of X_i(n) X_j(n)  of the real rows is G x G tiles of v_mfma_i32_16x16x64_i8, and
//     Re R[k][l] = Gm[2k][2l] + Gm[2k+1][2l+1]         Im R[k][l] = Gm[2k+1][2l] - Gm[2k][2l+1].
// Gm is symmetric, so the kernel computes the tiles (g, h) with g >= h only: group g's registers as operand A, group h's as operand B.
// On the diagonal A and B are the same registers and a transposed accumulator could not show; below it A != B, and the tile's
// orientation is part of the layout: A lane l feeds row l & 15, B lane l feeds column l & 15, D(row, col) is register row & 3 of lane
// col + 16 (row >> 2).  The scratch is Gm as [64][64] int64; entry (i, j) of an upper tile is read from (j, i) by the host.
#ifndef GPSIQ_STAP_GEOMETRY_H
#define GPSIQ_STAP_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kStapMaxElem = 8;                      // GPSIQ_ARRAY_MAX_ELEM (include/gpsiq_rows.h; gpsiq_stap.h asserts these three)
constexpr int kStapMaxTaps = 8;                      // GPSIQ_STAP_MAX_TAPS
constexpr int kStapMaxRows = 32;                     // GPSIQ_STAP_MAX_ROWS: K = nelem * ntaps
constexpr int kStapRealRows = 2 * kStapMaxRows;      // rows of the real Gram matrix
constexpr int kStapTile = 16;                        // rows of a group: one side of a tile
constexpr int kStapMaxGroups = kStapRealRows / kStapTile;
constexpr int kStapTileWords = kStapTile * kStapTile;
constexpr int kStapGramWords = kStapRealRows * kStapRealRows;     // int64 words of the device scratch of either covariance kernel
constexpr int kStapThreads = 256, kStapWaves = kStapThreads / 64;
constexpr int kStapMaxShift = 24;                    // gpsiq_cfilter's (gpsiq_stap.cpp asserts it)
constexpr long kStapWeightSum = 65535;               // sum over the K weights of |re| + |im|: gpsiq_cfilter's bound

constexpr int stap_groups(int rows) { return (rows + 7) / 8; }                // G: 1 .. 4
constexpr int stap_tiles(int groups) { return groups * (groups + 1) / 2; }    // tiles (g, h), g >= h, in the order (0,0) (1,0) (1,1) (2,0) ...

// ---- stap_cov_mfma<G> ------------------------------------------------------------------------------------------------------------
constexpr int kStapK = 64;                           // samples of a k-step: one instruction per tile
constexpr int kStapLaneSamples = 16;                 // of them a lane feeds: 16 bytes of one row
// One k-step moves an entry by at most 64 * 128 * 128 = 2^20, so a wave adds its int32 accumulators into int64 after at most
// 2047 k-steps: 2047 * 2^20 = 2^31 - 2^20 fits, 2048 * 2^20 = 2^31 does not (every byte -128 meets it exactly): the array's bound.
constexpr int kStapFlushSteps = 2047;
static_assert((int64_t) kStapFlushSteps * kStapK * 128 * 128 <= (int64_t) INT32_MAX, "an int32 entry of a Gram tile would wrap before its flush");
static_assert((int64_t) (kStapFlushSteps + 1) * kStapK * 128 * 128 > (int64_t) INT32_MAX, "the flush bound is not the largest that holds");
// A workgroup takes ONE run of consecutive k-steps, its four waves every fourth of them; the run is the span's k-steps over
// kStapMaxGrid workgroups, at least kStapMinRunSteps, a multiple of the waves.  A workgroup ends in 256 G (G + 1) / 2 atomic adds at
// most, 2 560 at G = 4: the grid is half the array's, so that no more than 1.3 million of them meet in the 4 096 words of the scratch.
constexpr int kStapMinRunSteps = 64;
constexpr unsigned kStapMaxGrid = 512;
static_assert(kStapMinRunSteps % kStapWaves == 0, "a run is shared out evenly");

// ---- stap_cov_generic ------------------------------------------------------------------------------------------------------------
// A workgroup stages kStapChunk samples of every element, and the ntaps - 1 before them, in LDS as dwords (I low, Q high,
// sign-extended); the K^2 entries of R times `phases` are shared out over the lanes: K^2 < 256: a lane owns one entry and every
// (256 / K^2)-th sample of the chunk; else 1 .. 4 entries and every sample.  int8: a term |Ia Ib + Qa Qb| <= 2^15, and a lane sums at
// most kStapChunk of them in int32 before it adds them into int64.  int16: one term can be 2^31, so the sums are int64 throughout.
constexpr int kStapChunk = 256;
static_assert((int64_t) kStapChunk * 2 * 128 * 128 <= (int64_t) INT32_MAX, "an int32 partial of the generic kernel would wrap before its flush");
constexpr int kStapGenRun = 4096;                    // samples of a workgroup's run
constexpr unsigned kStapGenMaxGrid = 2048;
static_assert(kStapGenRun % kStapChunk == 0, "a run is whole chunks");
constexpr int kStapGenOwned = kStapMaxRows * kStapMaxRows / kStapThreads;     // entries a lane owns at most: 4
static_assert(kStapGenOwned * kStapThreads == kStapMaxRows * kStapMaxRows, "the largest matrix is shared out evenly");
constexpr int stap_gen_phases(int rows) { return rows * rows < kStapThreads ? kStapThreads / (rows * rows) : 1; }

// ---- stap_combine ----------------------------------------------------------------------------------------------------------------
// A lane owns a SLOT, 16 aligned bytes of dst: 8 samples of int8 output, 4 of int16 (the array's slot), and reads the slot's samples
// and the ntaps - 1 before them of every element.
constexpr int stap_slot_samples(int out_size) { return 16 / (2 * out_size); }
constexpr unsigned kStapCombMaxGrid = 8192;

}  // namespace gpsiq
#endif
