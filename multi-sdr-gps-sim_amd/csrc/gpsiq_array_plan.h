// gpsiq_array_plan.h -- the kernel, the grid and the scratch a gpsiq_array_cov / gpsiq_array_combine call (include/gpsiq_rows.h,
// "Array") takes, and the host's way from the device scratch to the covariance.  Host code only, and pure: no HIP, no environment
// (the GPSIQ_ARRAY_KERNEL override is an argument, read per call by the caller).  tests/array_plan.cpp pins every plan on the CPU
// and multiplies the Gram tile out against the direct complex sum.
// Not a device source: the geometry the kernels are compiled for is gpsiq_array_geometry.h.
#ifndef GPSIQ_ARRAY_PLAN_H
#define GPSIQ_ARRAY_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_array_geometry.h"

namespace gpsiq {

enum { kArrGeneric = 0, kArrMfma = 1, kArrCombine = 2 };     // array_cov_generic; array_cov_mfma; array_combine (gpsiq_array_last_plan)
enum { kArrAuto = 0, kArrForceGeneric = 1, kArrForceMfma = 2 };

// The matrix kernel is the default for an int8 covariance from this many elements on: the element counts at which
// profiles/array_rates.txt (MI355X, 26e6 samples) shows it the faster of the two.  Rows "cov int8 | E=2", "E=4" and "E=8": the matrix
// kernel takes 0.59, 0.33 and 0.16 of the generic kernel's time (0.067 against 0.114 ms, 0.070 against 0.209 ms, 0.103 against
// 0.640 ms), so it is the default at every element count that was measured; one element was not measured and stays with the generic
// kernel.
constexpr int kArrMfmaMinElem = 2;

struct ArrayCovPlan {
    bool     launch = false;
    int      kernel = kArrGeneric;
    unsigned grid = 0, threads = 0;
    uint64_t run = 0;        // of a workgroup: samples (generic) or k-steps (matrix)
    uint64_t runs = 0;       // runs of the span: the grid, one run a workgroup (matrix), or more than the grid (generic: taken in turn)
    uint64_t steps = 0;      // k-steps of the span (matrix kernel; 0 for the generic one)
};

// arguments in range (the caller has checked them); force: kArrAuto, or the kernel GPSIQ_ARRAY_KERNEL names -- taken where it can serve
inline ArrayCovPlan plan_array_cov(int nelem, int nsamp, int in_size, int force)
{
    ArrayCovPlan p;
    if (nsamp <= 0) return p;
    const bool can = in_size == 1;                                    // (the int16 matrix path: DESIGN.md 8n, priced, not attempted)
    const bool mfma = force == kArrForceGeneric ? false : force == kArrForceMfma ? can : can && nelem >= kArrMfmaMinElem;
    p.launch = true;
    p.threads = kArrThreads;
    if (mfma) {
        p.kernel = kArrMfma;
        p.steps = ((uint64_t) nsamp + kArrK - 1) / kArrK;
        uint64_t run = (p.steps + kArrMaxGrid - 1) / kArrMaxGrid;
        run = (run + kArrWaves - 1) / kArrWaves * kArrWaves;
        p.run = run < (uint64_t) kArrMinRunSteps ? (uint64_t) kArrMinRunSteps : run;
        p.runs = (p.steps + p.run - 1) / p.run;
        p.grid = (unsigned) p.runs;
    } else {
        p.run = kArrGenRun;
        p.runs = ((uint64_t) nsamp + kArrGenRun - 1) / kArrGenRun;
        p.grid = p.runs < kArrGenMaxGrid ? (unsigned) p.runs : kArrGenMaxGrid;
    }
    return p;
}

// The device scratch of a call, kArrGramWords int64 words, to cov [nelem][nelem][2].  The matrix kernel leaves the Gram tile
// G[i][j], row 2 e + c the component c of element e; the generic kernel leaves R itself as [8][8][2], the entry (a, b) of its
// pw x pw matrix at words 16 a + 2 b (the stride is the tile's whatever pw was).
inline void array_scratch_to_cov(int kernel, const int64_t *scratch, int nelem, int64_t *cov)
{
    for (int a = 0; a < nelem; ++a)
        for (int b = 0; b < nelem; ++b) {
            int64_t *out = cov + 2 * ((size_t) a * (size_t) nelem + (size_t) b);
            if (kernel == kArrMfma) {
                const auto g = [&](int i, int j) { return scratch[i * kArrRows + j]; };
                out[0] = g(2 * a, 2 * b) + g(2 * a + 1, 2 * b + 1);
                out[1] = g(2 * a + 1, 2 * b) - g(2 * a, 2 * b + 1);
            } else {
                out[0] = scratch[2 * kArrMaxElem * a + 2 * b];
                out[1] = scratch[2 * kArrMaxElem * a + 2 * b + 1];
            }
        }
}

struct ArrayCombinePlan {
    bool     launch = false;
    unsigned grid = 0, threads = 0;
    int      lead = 0;       // samples of the first slot that lie before sample 0
    uint64_t slots = 0;      // 16-byte slots of dst the span touches
};

// dst_low4: the low four bits of dst's address (4-byte aligned: the caller has checked it)
inline ArrayCombinePlan plan_array_combine(int nsamp, int out_size, unsigned dst_low4)
{
    ArrayCombinePlan p;
    if (nsamp <= 0) return p;
    const int S = array_slot_samples(out_size);
    p.launch = true;
    p.threads = kArrThreads;
    p.lead = (int) (dst_low4 & 15u) / (2 * out_size);
    p.slots = ((uint64_t) nsamp + (uint64_t) p.lead + (uint64_t) S - 1) / (uint64_t) S;
    const uint64_t groups = (p.slots + kArrThreads - 1) / kArrThreads;
    p.grid = groups < kArrCombMaxGrid ? (unsigned) groups : kArrCombMaxGrid;
    return p;
}

// sum over e of |re_e| + |im_e| of weights [nelem][2]
inline long array_weight_sum(const int16_t *re_im, int nelem)
{
    long mag = 0;
    for (int k = 0; k < 2 * nelem; ++k) mag += re_im[k] < 0 ? -(long) re_im[k] : (long) re_im[k];
    return mag;
}

}  // namespace gpsiq
#endif
