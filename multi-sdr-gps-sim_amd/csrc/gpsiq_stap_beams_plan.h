// gpsiq_stap_beams_plan.h -- the kernel, the padding, the grid and the matrix kernel's operand a gpsiq_stap_beams call
// (include/gpsiq_rows.h, "Space-time array") takes.  Host code only, and pure: no HIP, no environment (the GPSIQ_STAP_BEAMS_KERNEL
// override is an argument, read per call by the caller).  tests/stap_beams_plan.cpp pins every plan on the CPU, multiplies the planes out
// against the weights and models one tile of the matrix kernel.
// Not a device source: the geometry the kernels are compiled for is gpsiq_stap_beams_geometry.h.
#ifndef GPSIQ_STAP_BEAMS_PLAN_H
#define GPSIQ_STAP_BEAMS_PLAN_H

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "gpsiq_stap_beams_geometry.h"
#include "gpsiq_stap_plan.h"

namespace gpsiq {

enum { kBeamsGeneric = 0, kBeamsMfma = 1 };          // stap_beams_generic; stap_beams_mfma (gpsiq_stap_beams_last_plan)
enum { kBeamsAuto = 0, kBeamsForceGeneric = 1, kBeamsForceMfma = 2 };

// The matrix kernel is the default, where it can serve, from this many padded rows K' = nelem * TP on, by the number of beams and the
// input format: the smallest measured K' from which it is the faster of the two at every measured row of that size or larger with at
// least that many beams.  profiles/stap_beams_rates.txt (MI355X, 26e6 samples, K' = 2, 8, 16, 32 and 32 at 2 x 1, 2 x 4, 4 x 4, 4 x 8 and
// 8 x 4; 1, 2, 4 and 8 beams), column "matrix / generic":
//   int8 -> int8     8 beams: 0.69, 0.46, 0.36, 0.25, 0.29 -- from 2 rows.   4 beams: 1.20, 0.80, 0.63, 0.45, 0.54 -- from 8 rows.
//                    2 beams: 2.19, 1.46, 1.13, 0.80, 1.02 -- the two shapes of 32 rows disagree: generic.   1 beam: 3.73 to 1.43: generic.
//   int16 -> int16   8 beams: 1.03, 0.70, 0.54, 0.34, 0.39 -- from 8 rows.   4 beams: 1.68, 1.15, 0.90, 0.59, 0.71 -- from 16 rows.
//                    2 beams: 3.02 to 1.09, 1 beam: 5.21 to 2.03: generic.
// The two rows nearest to 1 are apart by more than their spread (the file's last two columns): int8 8 x 4 x 2, generic 0.807 .. 0.816 ms
// against matrix 0.822 .. 0.829; int16 2 x 1 x 8, 0.536 .. 0.541 against 0.554 .. 0.560.
// 3 beams follow 2, and 5 to 7 follow 4: not measured.  The matrix kernel's time hardly moves with the beams (0.310 to 0.389 ms at 2 x 4
// int8), the generic kernel's is nbeams calls of stap_combine (0.80 to 1.05 of them): with one beam the matrix kernel does not beat
// stap_combine at any measured shape (1.45 to 5.14 of its time).  kBeamsNever: above every legal K'.
constexpr int kBeamsNever = 2 * kStapMaxRows;
constexpr int beams_mfma_min_rows(int in_size, int nbeams)
{
    return nbeams >= 8 ? (in_size == 1 ? 2 : 8) : nbeams >= 4 ? (in_size == 1 ? 8 : 16) : kBeamsNever;
}

struct BeamsStats { long mag = 0; int max_entry = -32768; };          // of one beam: the bound's sum, the largest of re, +im, -im

inline BeamsStats beams_weight_stats(const int16_t *re_im /* [rows][2] */, int rows)
{
    BeamsStats st;
    st.mag = stap_weight_sum(re_im, rows);
    for (int k = 0; k < rows; ++k) {
        const int re = re_im[2 * k], im = re_im[2 * k + 1];
        const int m = re > im ? (re > -im ? re : -im) : (im > -im ? im : -im);
        if (m > st.max_entry) st.max_entry = m;
    }
    return st;
}

struct BeamsPlan {
    bool     launch = false;
    int      kernel = kBeamsGeneric;
    int      padded = 0;     // TP of the matrix kernel (0 for the generic one)
    unsigned grid = 0, threads = 0;
    int      run = 0;        // samples of a workgroup's run: a chunk (matrix), or the slots of its threads (generic)
    uint64_t runs = 0;       // runs of the span, taken in turn by the grid
};

// whether the matrix kernel can serve: the shape pads into 32 rows and every entry of the operand splits into two signed bytes
inline bool beams_mfma_serves(int nelem, int ntaps, int max_entry) { return beams_padded_taps(nelem, ntaps) > 0 && max_entry <= kBeamsMaxEntry; }

// arguments in range (the caller has checked them); max_entry: the largest of re, +im, -im over every beam's weights; force: kBeamsAuto,
// or the kernel GPSIQ_STAP_BEAMS_KERNEL names -- taken where it can serve
inline BeamsPlan plan_stap_beams(int nelem, int ntaps, int nbeams, int nsamp, int in_size, int out_size, int max_entry, int force)
{
    BeamsPlan p;
    if (nsamp <= 0) return p;
    const bool can = beams_mfma_serves(nelem, ntaps, max_entry);
    const int tp = beams_padded_taps(nelem, ntaps);
    const bool mfma = force == kBeamsForceGeneric ? false : force == kBeamsForceMfma ? can : can && nelem * tp >= beams_mfma_min_rows(in_size, nbeams);
    p.launch = true;
    p.threads = kBeamsThreads;
    if (mfma) {
        p.kernel = kBeamsMfma;
        p.padded = tp;
        p.run = beams_chunk_samples(out_size);
        p.runs = ((uint64_t) nsamp + (uint64_t) p.run - 1) / (uint64_t) p.run;
        p.grid = p.runs < kBeamsMaxGrid ? (unsigned) p.runs : kBeamsMaxGrid;
    } else {
        p.run = kBeamsThreads * beams_lane_samples(out_size);
        p.runs = ((uint64_t) nsamp + (uint64_t) p.run - 1) / (uint64_t) p.run;
        p.grid = p.runs < kBeamsGenMaxGrid ? (unsigned) p.runs : kBeamsGenMaxGrid;
    }
    return p;
}

// entry (row, k) of A from the weights w [nbeams][nelem][ntaps][2] (gpsiq_stap_beams_geometry.h): row 2 b meets re at the byte of I and
// -im at the byte of Q, row 2 b + 1 meets im and re there
inline int beams_entry(const int16_t *w, int nelem, int ntaps, int nbeams, int tp, int row, int k)
{
    const int b = row >> 1, e = k / (2 * tp), t = tp - 1 - (k % (2 * tp)) / 2, c = k & 1;
    if (b >= nbeams || e >= nelem || t >= ntaps) return 0;
    const int16_t *v = w + 2 * (((size_t) b * (size_t) nelem + (size_t) e) * (size_t) ntaps + (size_t) t);
    const int re = v[0], im = v[1];
    return row & 1 ? (c ? re : im) : (c ? -im : re);
}

// What the host sends ahead of a launch, kBeamsCoefDwords dwords: the two digit planes of A in fragment order (lane l = (row l & 15,
// group l >> 4) holds bytes k = 16 (l >> 4) + j at 16 l + j), the row constants 128 sum_k A(row, k), and the weights as dwords
// [kBeamsMax][kStapMaxRows] (re low, im high).  tp == 0 (the generic kernel serves): planes and constants stay zero.
inline void beams_build_coef(const int16_t *w, int nelem, int ntaps, int nbeams, int tp, uint32_t *coef)
{
    std::memset(coef, 0, sizeof(uint32_t) * kBeamsCoefDwords);
    int8_t *planes = reinterpret_cast<int8_t *>(coef);
    int32_t *consts = reinterpret_cast<int32_t *>(coef + kBeamsConstAt);
    if (tp)
        for (int row = 0; row < kBeamsRows; ++row) {
            long sum = 0;
            for (int k = 0; k < kBeamsK; ++k) {
                const int entry = beams_entry(w, nelem, ntaps, nbeams, tp, row, k);
                const int d0 = ((entry + 128) & 255) - 128, d1 = (entry - d0) / 256;
                const size_t at = (size_t) (16 * (k / 16) + row) * 16 + (size_t) (k % 16);
                planes[at] = (int8_t) d0;
                planes[kBeamsPlaneBytes + at] = (int8_t) d1;
                sum += entry;
            }
            consts[row] = (int32_t) (128 * sum);                     // |.| <= 128 * 65535 < 2^23
        }
    const int rows = nelem * ntaps;
    for (int b = 0; b < nbeams; ++b)
        for (int r = 0; r < rows; ++r) {
            const int16_t *v = w + 2 * ((size_t) b * (size_t) rows + (size_t) r);
            coef[kBeamsWeightsAt + b * kStapMaxRows + r] = (uint32_t) (uint16_t) v[0] | ((uint32_t) (uint16_t) v[1] << 16);
        }
}

}  // namespace gpsiq
#endif
