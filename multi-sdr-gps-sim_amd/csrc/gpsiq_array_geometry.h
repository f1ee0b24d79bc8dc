// gpsiq_array_geometry.h -- the constants the kernels of gpsiq_array_cov / gpsiq_array_combine (gpsiq_array_kernels.hip) are compiled for
// and the host plans with (gpsiq_array_plan.h): the Gram tile of the matrix kernel, the runs, the flush bound, the slot of the
// combiner.  A device source (behind gpsiq_kernels_id()); no HIP in it, so tests/array_plan.cpp includes it with the host compiler.
//
// The Gram tile.  With E <= 8 elements the 2 E real rows  I_0, Q_0, I_1, Q_1, ... (row 2 e + c: component c of element e)  are the 16
// rows of one v_mfma_i32_16x16x64_i8 tile, rows of absent elements all zero.  One instruction with the SAME 64 samples as operand A and
// as operand B adds  G[i][j] += sum over the 64 samples of X_i X_j  to all 256 entries, and
//     Re R[a][b] = G[2a][2b] + G[2a+1][2b+1]         Im R[a][b] = G[2a+1][2b] - G[2a][2b+1].
// Both operands are the same registers, so the order of the 64 samples inside a k-step cannot matter, and G is symmetric, so neither
// can a transposed accumulator: what the layout has to get right is which lane feeds which row, and which register holds which entry.
#ifndef GPSIQ_ARRAY_GEOMETRY_H
#define GPSIQ_ARRAY_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kArrMaxElem = 8;                       // GPSIQ_ARRAY_MAX_ELEM (include/gpsiq_rows.h; gpsiq_array.h asserts it)
constexpr int kArrRows = 2 * kArrMaxElem;            // rows of the Gram tile
constexpr int kArrGramWords = kArrRows * kArrRows;   // int64 words of the device scratch of either covariance kernel
constexpr int kArrThreads = 256, kArrWaves = kArrThreads / 64;
constexpr int kArrMaxShift = 24;                     // gpsiq_cfilter's (gpsiq_array.cpp asserts it)
constexpr long kArrWeightSum = 65535;                // sum over e of |re_e| + |im_e|: gpsiq_cfilter's bound

// ---- array_cov_mfma --------------------------------------------------------------------------------------------------------------
constexpr int kArrK = 64;                            // samples of a k-step: one instruction
constexpr int kArrLaneSamples = 16;                  // of them a lane feeds: 16 bytes of one row
// One k-step moves an entry by at most 64 * 128 * 128 = 2^20, so a wave adds its int32 accumulators into int64 after at most
// 2047 k-steps: 2047 * 2^20 = 2^31 - 2^20 fits, 2048 * 2^20 = 2^31 does not (every element all -128 meets it exactly).
constexpr int kArrFlushSteps = 2047;
static_assert((int64_t) kArrFlushSteps * kArrK * 128 * 128 <= (int64_t) INT32_MAX, "an int32 entry of the Gram tile would wrap before its flush");
static_assert((int64_t) (kArrFlushSteps + 1) * kArrK * 128 * 128 > (int64_t) INT32_MAX, "the flush bound is not the largest that holds");
// A workgroup takes ONE run of consecutive k-steps, its four waves every fourth of them; the run is the span's k-steps over
// kArrMaxGrid workgroups, at least kArrMinRunSteps, a multiple of the waves.
constexpr int kArrMinRunSteps = 64;
constexpr unsigned kArrMaxGrid = 1024;
static_assert(kArrMinRunSteps % kArrWaves == 0, "a run is shared out evenly");

// ---- array_cov_generic -----------------------------------------------------------------------------------------------------------
// A workgroup stages kArrChunk samples of every element in LDS as dwords (I low, Q high, sign-extended); a lane owns one entry
// R[a][b] of a pw x pw matrix, pw = 2, 4 or 8 the least that holds the elements, and every (256 / pw^2)-th sample of the chunk.
// int8: a term |Ia Ib + Qa Qb| <= 2^15, and a lane sums at most kArrChunk of them in int32 before it adds them into int64:
// kArrChunk * 2^15 = 2^23.  int16: one term can be 2^31, so the sums are int64 throughout.
constexpr int kArrChunk = 256;
static_assert((int64_t) kArrChunk * 2 * 128 * 128 <= (int64_t) INT32_MAX, "an int32 partial of the generic kernel would wrap before its flush");
constexpr int kArrGenRun = 4096;                     // samples of a workgroup's run
constexpr unsigned kArrGenMaxGrid = 2048;
static_assert(kArrGenRun % kArrChunk == 0, "a run is whole chunks");
constexpr int array_pair_width(int nelem) { return nelem <= 2 ? 2 : nelem <= 4 ? 4 : 8; }

// ---- array_combine ---------------------------------------------------------------------------------------------------------------
// A lane owns a SLOT, 16 aligned bytes of dst: 8 samples of int8 output, 4 of int16 (gpsiq_mix_geometry.h has the same slot).
constexpr int array_slot_samples(int out_size) { return 16 / (2 * out_size); }
constexpr unsigned kArrCombMaxGrid = 8192;

}  // namespace gpsiq
#endif
