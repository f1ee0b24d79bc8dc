// gpsiq_cfilter_plan.h -- the kernel and the grid a gpsiq_cfilter call (include/gpsiq_rows.h, "Complex filter and notch") takes, and the
// matrix kernels' operand as the host builds it.  Host code only, and pure: no HIP, no environment (the GPSIQ_CFILTER_KERNEL override
// is an argument, read per call by the caller).  The output count and next_phase are gpsiq_filter's (filter_span, gpsiq_filter_plan.h).
// tests/cfilter_plan.cpp pins every plan on the CPU and multiplies the planes out against the direct sum.
// Not a device source: the geometry the kernels are compiled for is gpsiq_cfilter_geometry.h.
#ifndef GPSIQ_CFILTER_PLAN_H
#define GPSIQ_CFILTER_PLAN_H

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "gpsiq_cfilter_geometry.h"
#include "gpsiq_filter_plan.h"

namespace gpsiq {

enum { kCfiltGeneric = 0, kCfiltMfma = 1, kCfiltMfma16 = 2 };       // cfilter_generic; filter_mfma with complex planes; cfilter_mfma16
enum { kCfiltAuto = 0, kCfiltForceGeneric = 1, kCfiltForceMfma = 2 };

// The matrix kernel is the default from this many taps on, where it can serve: one threshold per input format, each the smallest
// measured ntaps from which the matrix kernel is the faster of the two at every larger measured row of profiles/cfilter_rates.txt
// (MI355X, 26e6 samples, 5 to 257 taps, decim 1 and 4).  int8 input: filter_mfma with complex planes is the faster at every measured
// row, 0.78 to 0.86 of the generic kernel's time at 5 taps and 0.07 to 0.13 at 257, and takes gpsiq_filter's own time for real taps of
// the same length; below 5 taps nothing was measured and the generic kernel stays.  int16 input: cfilter_mfma16 is the faster at every
// row from 17 taps on, 0.63 to 0.85 of the generic kernel's time at 17 taps and 0.12 to 0.18 at 257; at 5 taps it is the slower
// (1.04 to 1.09) and at 9 taps the two tie at decim 4 (1.01), so the generic kernel keeps those.
constexpr int kCfiltMfmaMinTaps8 = 5;
constexpr int kCfiltMfmaMinTaps16 = 17;

struct CtapStats { long mag = 0; int max_re = -32768, max_im = -32768, min_im = 32767; };

inline CtapStats cfilter_tap_stats(const int16_t *re_im /* [ntaps][2] */, int ntaps)
{
    CtapStats st;
    for (int k = 0; k < ntaps; ++k) {
        const int re = re_im[2 * k], im = re_im[2 * k + 1];
        st.mag += (re < 0 ? -(long) re : (long) re) + (im < 0 ? -(long) im : (long) im);
        if (re > st.max_re) st.max_re = re;
        if (im > st.max_im) st.max_im = im;
        if (im < st.min_im) st.min_im = im;
    }
    return st;
}

// whether the matrix kernels can serve: every entry of the operand (re, +im, -im) inside two signed bytes
inline bool cfilter_mfma_serves(const CtapStats &st) { return st.max_re <= kFiltMfmaMaxTap && st.max_im <= kFiltMfmaMaxTap && -st.min_im <= kFiltMfmaMaxTap; }

// FilterPlan (gpsiq_filter_plan.h) with kernel one of kCfilt*: arguments in range (the caller has checked them); force: kCfiltAuto, or
// the path GPSIQ_CFILTER_KERNEL names -- taken where it can serve
inline FilterPlan plan_cfilter(int nsamp, int in_size, int ntaps, int decim, int phase, const CtapStats &st, int force)
{
    FilterPlan p;
    filter_span(nsamp, decim, phase, &p.nout, &p.next_phase);
    if (p.nout <= 0) return p;
    const int run16 = in_size == 2 ? cfilter_mfma16_run(ntaps, decim) : 0;
    const bool can = cfilter_mfma_serves(st) && (in_size == 1 || run16 > 0);
    const int min_taps = in_size == 1 ? kCfiltMfmaMinTaps8 : kCfiltMfmaMinTaps16;
    const bool mfma = force == kCfiltForceGeneric ? false : force == kCfiltForceMfma ? can : can && ntaps >= min_taps;
    p.launch = true;
    p.threads = kFiltThreads;
    if (mfma) {
        p.steps = filter_mfma_steps(ntaps, decim);
        if (in_size == 1) {
            p.kernel = kCfiltMfma;
            p.run = filter_mfma_run(ntaps, decim);
            p.lds = (size_t) filter_mfma_plane_bytes(p.steps) + (size_t) filter_mfma_window_bytes(p.run, decim, p.steps);
        } else {
            p.kernel = kCfiltMfma16;
            p.run = run16;
            p.lds = (size_t) cfilter_mfma16_lds(p.run, decim, p.steps);
        }
    } else {
        p.kernel = kCfiltGeneric;
        p.run = filter_generic_run(ntaps, decim);
        p.lds = 4 * ((size_t) (p.run - 1) * (size_t) decim + (size_t) ntaps) + 4 * (size_t) ntaps;
    }
    p.runs = ((uint64_t) p.nout + (uint64_t) p.run - 1) / (uint64_t) p.run;
    p.grid = p.runs < kFiltMaxGrid ? (unsigned) p.runs : kFiltMaxGrid;
    return p;
}

// The two digit planes of the matrix kernels in fragment order (gpsiq_filter_geometry.h): lane l = (row i = l & 15, group g = l >> 4)
// of k-step t holds bytes j = 0..15, k = 64 t + 16 g + j, of A(i, k) (gpsiq_cfilter_geometry.h).  planes: [2][steps * 1024] bytes.
inline void cfilter_build_planes(const int16_t *re_im, int ntaps, int decim, int steps, int8_t *planes)
{
    const size_t plane = (size_t) steps * kFiltK * 16;
    std::memset(planes, 0, 2 * plane);
    const auto put = [&](int i, int kk, int entry) {
        const int t = kk / kFiltK, g = (kk % kFiltK) / 16, j = kk % 16;
        const size_t at = ((size_t) t * 64 + (size_t) (16 * g + i)) * 16 + (size_t) j;
        const int d0 = ((entry + 128) & 255) - 128, d1 = (entry - d0) / 256;
        planes[at] = (int8_t) d0;
        planes[plane + at] = (int8_t) d1;
    };
    for (int jj = 0; jj < kFiltColOutputs; ++jj)
        for (int tap = 0; tap < ntaps; ++tap) {
            const int k_i = 2 * jj * decim + 2 * (ntaps - 1) - 2 * tap, re = re_im[2 * tap], im = re_im[2 * tap + 1];
            put(2 * jj, k_i, re);
            put(2 * jj, k_i + 1, -im);
            put(2 * jj + 1, k_i + 1, re);
            put(2 * jj + 1, k_i, im);
        }
}

// cfilter_mfma16's per-row constants 128 sum_k A(row, k), by the row's component: |.| <= 128 * 65535 < 2^23
inline void cfilter_row_consts(const int16_t *re_im, int ntaps, int32_t out[2])
{
    long sre = 0, sim = 0;
    for (int k = 0; k < ntaps; ++k) { sre += re_im[2 * k]; sim += re_im[2 * k + 1]; }
    out[0] = (int32_t) (128 * (sre - sim));
    out[1] = (int32_t) (128 * (sre + sim));
}

}  // namespace gpsiq
#endif
