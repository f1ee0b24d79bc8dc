// gpsiq_stap_plan.h -- the kernel, the row groups, the grid and the scratch a gpsiq_stap_cov / gpsiq_stap_combine call
// (include/gpsiq_rows.h, "Space-time array") takes, and the host's way from the device scratch to the covariance, the mirror of the
// upper tiles included.  Host code only, and pure: no HIP, no environment (the GPSIQ_STAP_KERNEL override is an argument, read per call
// by the caller).  tests/stap_plan.cpp pins every plan on the CPU and multiplies the tiles out against the direct complex sums.
// Not a device source: the geometry the kernels are compiled for is gpsiq_stap_geometry.h.
#ifndef GPSIQ_STAP_PLAN_H
#define GPSIQ_STAP_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_stap_geometry.h"

namespace gpsiq {

enum { kStapGeneric = 0, kStapMfma = 1, kStapCombine = 2 };  // stap_cov_generic; stap_cov_mfma; stap_combine (gpsiq_stap_last_plan)
enum { kStapAuto = 0, kStapForceGeneric = 1, kStapForceMfma = 2 };

// The matrix kernel is the default for an int8 covariance from this many rows K = nelem * ntaps on.  profiles/stap_rates.txt (MI355X,
// 26e6 samples), rows "cov int8 | 2 x 1", "2 x 2", "2 x 4", "4 x 2", "4 x 4", "4 x 8" and "8 x 4": the matrix kernel takes 0.76, 0.49,
// 0.23, 0.20, 0.13, 0.10 and 0.13 of the generic kernel's time (0.113 against 0.150 ms, 0.129 against 0.263, 0.140 against 0.609,
// 0.132 against 0.653, 0.282 against 2.204, 0.862 against 8.477, 1.156 against 8.759), so it is the default at every shape that was
// measured, 2 to 32 rows.  One row was not measured and stays with the generic kernel, as one element does in the array stage.
constexpr int kStapMfmaMinRows = 2;

struct StapCovPlan {
    bool     launch = false;
    int      kernel = kStapGeneric;
    int      groups = 0;     // G of the matrix kernel (0 for the generic one)
    unsigned grid = 0, threads = 0;
    uint64_t run = 0;        // of a workgroup: samples (generic) or k-steps (matrix)
    uint64_t runs = 0;       // runs of the span: the grid, one run a workgroup (matrix), or more than the grid (generic: taken in turn)
    uint64_t steps = 0;      // k-steps of the span (matrix kernel; 0 for the generic one)
};

// arguments in range (the caller has checked them); force: kStapAuto, or the kernel GPSIQ_STAP_KERNEL names -- taken where it can serve
inline StapCovPlan plan_stap_cov(int nelem, int ntaps, int nsamp, int in_size, int force)
{
    StapCovPlan p;
    if (nsamp <= 0) return p;
    const int rows = nelem * ntaps;
    const bool can = in_size == 1;                                    // (an int16 matrix path: out of scope, as the array's)
    const bool mfma = force == kStapForceGeneric ? false : force == kStapForceMfma ? can : can && rows >= kStapMfmaMinRows;
    p.launch = true;
    p.threads = kStapThreads;
    if (mfma) {
        p.kernel = kStapMfma;
        p.groups = stap_groups(rows);
        p.steps = ((uint64_t) nsamp + kStapK - 1) / kStapK;
        // (kStapMaxGrid, 512, is NOT measured: no second grid size was run, so whether the workgroups' atomics show in the rates at
        // G = 4 is open -- DESIGN.md 8o; the note stands here because the constant's own header is behind gpsiq_kernels_id())
        uint64_t run = (p.steps + kStapMaxGrid - 1) / kStapMaxGrid;
        run = (run + kStapWaves - 1) / kStapWaves * kStapWaves;
        p.run = run < (uint64_t) kStapMinRunSteps ? (uint64_t) kStapMinRunSteps : run;
        p.runs = (p.steps + p.run - 1) / p.run;
        p.grid = (unsigned) p.runs;
    } else {
        p.run = kStapGenRun;
        p.runs = ((uint64_t) nsamp + kStapGenRun - 1) / kStapGenRun;
        p.grid = p.runs < kStapGenMaxGrid ? (unsigned) p.runs : kStapGenMaxGrid;
    }
    return p;
}

// Entry (i, j) of the real Gram matrix from the matrix kernel's scratch [64][64]: the kernel writes the tiles on and below the
// diagonal, and an entry of an upper tile is its mirror
inline int64_t stap_gram_entry(const int64_t *scratch, int i, int j)
{
    return i / kStapTile >= j / kStapTile ? scratch[i * kStapRealRows + j] : scratch[j * kStapRealRows + i];
}

// The device scratch of a call, kStapGramWords int64 words, to cov [K][K][2].  The matrix kernel leaves the Gram matrix of the real
// rows 2 k + c (above); the generic kernel leaves R itself, entry (k, l) at words 2 (k K + l).
inline void stap_scratch_to_cov(int kernel, const int64_t *scratch, int rows, int64_t *cov)
{
    for (int k = 0; k < rows; ++k)
        for (int l = 0; l < rows; ++l) {
            int64_t *out = cov + 2 * ((size_t) k * (size_t) rows + (size_t) l);
            if (kernel == kStapMfma) {
                const auto g = [&](int i, int j) { return stap_gram_entry(scratch, i, j); };
                out[0] = g(2 * k, 2 * l) + g(2 * k + 1, 2 * l + 1);
                out[1] = g(2 * k + 1, 2 * l) - g(2 * k, 2 * l + 1);
            } else {
                out[0] = scratch[2 * (k * rows + l)];
                out[1] = scratch[2 * (k * rows + l) + 1];
            }
        }
}

struct StapCombinePlan {
    bool     launch = false;
    unsigned grid = 0, threads = 0;
    int      lead = 0;       // samples of the first slot that lie before sample 0
    uint64_t slots = 0;      // 16-byte slots of dst the span touches
};

// dst_low4: the low four bits of dst's address (4-byte aligned: the caller has checked it)
inline StapCombinePlan plan_stap_combine(int nsamp, int out_size, unsigned dst_low4)
{
    StapCombinePlan p;
    if (nsamp <= 0) return p;
    const int S = stap_slot_samples(out_size);
    p.launch = true;
    p.threads = kStapThreads;
    p.lead = (int) (dst_low4 & 15u) / (2 * out_size);
    p.slots = ((uint64_t) nsamp + (uint64_t) p.lead + (uint64_t) S - 1) / (uint64_t) S;
    const uint64_t groups = (p.slots + kStapThreads - 1) / kStapThreads;
    p.grid = groups < kStapCombMaxGrid ? (unsigned) groups : kStapCombMaxGrid;
    return p;
}

// sum over the rows of |re| + |im| of weights [rows][2]
inline long stap_weight_sum(const int16_t *re_im, int rows)
{
    long mag = 0;
    for (int k = 0; k < 2 * rows; ++k) mag += re_im[k] < 0 ? -(long) re_im[k] : (long) re_im[k];
    return mag;
}

}  // namespace gpsiq
#endif
