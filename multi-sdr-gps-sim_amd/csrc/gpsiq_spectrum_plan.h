// gpsiq_spectrum_plan.h -- the segments, the bound, the kernel and the grid a gpsiq_spectrum call (include/gpsiq_rows.h, "Spectrum")
// takes.  Host code only, and pure: no HIP, no environment (the GPSIQ_SPECTRUM_KERNEL override is an argument, read per call by the
// caller).  tests/spectrum_plan.cpp pins every plan on the CPU.  Not a device source: the geometry the kernels are compiled for is
// gpsiq_spectrum_geometry.h.
#ifndef GPSIQ_SPECTRUM_PLAN_H
#define GPSIQ_SPECTRUM_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_spectrum_geometry.h"

namespace gpsiq {

inline bool spectrum_shape_ok(int nfft, int hop, int window, int navg)
{
    return (nfft == 64 || nfft == 128 || nfft == 256 || nfft == 512) && (hop == nfft || hop == nfft / 2) && (window == 0 || window == 1) && navg >= 1;
}

// segments and whole groups of a span (include/gpsiq_rows.h: gpsiq_spectrum_span); arguments in range
inline void spectrum_span(int nsamp, int nfft, int hop, int navg, int *nseg, int *ngroups)
{
    *nseg = nsamp < nfft ? 0 : (nsamp - nfft) / hop + 1;
    *ngroups = *nseg / navg;
}

// the bound of the contract: 2 navg Ys^2 <= 2^64 - 1 with Ymax = W N 500 xmax, in 128 bits (Ymax < 2^36, navg < 2^31: 2^104 at most)
inline bool spectrum_fits(int sample_size, int nfft, int window, int navg, int shift)
{
    const unsigned __int128 ymax = (unsigned __int128) (window ? 4 : 1) * (unsigned) nfft * 500u * (sample_size == 1 ? 128u : 32768u);
    const unsigned __int128 ys = shift == 0 ? ymax : (ymax >> shift) + 1;
    return (unsigned __int128) 2 * (unsigned) navg * ys * ys <= (unsigned __int128) UINT64_MAX;
}

// the smallest shift in 0..kSpecMaxShift that fits, -1 if none does
inline int spectrum_min_shift(int sample_size, int nfft, int window, int navg)
{
    for (int s = 0; s <= kSpecMaxShift; ++s)
        if (spectrum_fits(sample_size, nfft, window, navg, s)) return s;
    return -1;
}

enum { kSpecGeneric = 0, kSpecMfma = 1 };
enum { kSpecAuto = 0, kSpecForceGeneric = 1, kSpecForceMfma = 2 };

// Whether the matrix kernel is the default where it can serve.  profiles/spectrum_rates.txt (MI355X, 26e6 int8 samples in one group, median
// kernel_ms of nine calls, the two kernels alternating in one run): it is the faster of the two at every measured row -- every nfft,
// both hops, both windows -- by 8 to 14 times, so it is the default for every int8 call.
constexpr bool kSpecMfmaDefault = true;

struct SpectrumPlan {
    bool     launch = false;           // false: no whole group, nothing is launched
    int      kernel = kSpecGeneric;
    int      nseg = 0, ngroups = 0;
    unsigned grid = 0, threads = 0;
    int      run = 0;                  // generic: segments of a unit at most; matrix kernel: segments of a pass
    uint64_t per = 0;                  // generic: units of a group; matrix kernel: passes of a workgroup
    uint64_t work = 0;                 // generic: units of the launch (workgroup w takes w, w + grid, ...); matrix kernel: its passes
    size_t   lds = 0;                  // dynamic LDS of the launch, bytes
    size_t   power_bytes = 0;          // the device result
};

// whether the matrix kernel can serve: an int8 input
inline bool spectrum_mfma_serves(int sample_size) { return sample_size == 1; }

// arguments in range (the caller has checked them); force: kSpecAuto, or the path GPSIQ_SPECTRUM_KERNEL names -- taken where it can serve
inline SpectrumPlan plan_spectrum(int nsamp, int sample_size, int nfft, int hop, int navg, int force)
{
    SpectrumPlan p;
    spectrum_span(nsamp, nfft, hop, navg, &p.nseg, &p.ngroups);
    if (p.ngroups <= 0) return p;
    const bool can = spectrum_mfma_serves(sample_size);
    const bool mfma = force == kSpecForceGeneric ? false : force == kSpecForceMfma ? can : can && kSpecMfmaDefault;
    const uint64_t used = (uint64_t) p.ngroups * (uint64_t) navg;          // the segments that are read
    p.launch = true;
    p.power_bytes = (size_t) p.ngroups * (size_t) nfft * sizeof(uint64_t);
    if (mfma) {
        p.kernel = kSpecMfma;
        p.threads = kSpecThreads;
        p.run = spectrum_mfma_cols(nfft, hop);
        p.work = (used + (uint64_t) p.run - 1) / (uint64_t) p.run;
        p.per = (p.work + kSpecMfmaGrid - 1) / kSpecMfmaGrid;
        p.grid = (unsigned) ((p.work + p.per - 1) / p.per);
        p.lds = (size_t) spectrum_mfma_sums_bytes(nfft) + (size_t) spectrum_window_bytes(nfft, hop, p.run);
    } else {
        p.threads = (unsigned) spectrum_generic_threads(nfft);
        p.run = kSpecRun;
        p.per = ((uint64_t) navg + kSpecRun - 1) / kSpecRun;
        p.work = (uint64_t) p.ngroups * p.per;
        p.grid = p.work < kSpecMaxGrid ? (unsigned) p.work : kSpecMaxGrid;
    }
    return p;
}

}  // namespace gpsiq
#endif
