// gpsiq_filter_plan.h -- the output count, the kernel and the grid a gpsiq_filter call (include/gpsiq_rows.h, "Filter") takes.  Host
// code only, and pure: no HIP, no environment (the GPSIQ_FILTER_KERNEL override is an argument, read per call by the caller; so is
// GPSIQ_FILTER_PIECE_BLOCKS, for the piece size of gpsiq_generate_batch_filtered: stage_piece_blocks, gpsiq_pieces.h).
// The matrix kernel's operand as the host builds it is here too (filter_build_planes).  tests/filter_plan.cpp pins every plan on the
// CPU and multiplies the planes out against the direct sum.
// Not a device source: the geometry the kernels are compiled for is gpsiq_filter_geometry.h.
#ifndef GPSIQ_FILTER_PLAN_H
#define GPSIQ_FILTER_PLAN_H

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "gpsiq_filter_geometry.h"
#include "gpsiq_pieces.h"

namespace gpsiq {

// outputs of a span and the phase its continuation starts at (include/gpsiq_rows.h: gpsiq_filter_span); arguments in range
inline void filter_span(int nsamp, int decim, int phase, int *nout, int *next_phase)
{
    const int64_t n = phase >= nsamp ? 0 : ((int64_t) nsamp - phase + decim - 1) / decim;
    *nout = (int) n;
    *next_phase = (int) ((int64_t) phase + n * decim - nsamp);
}

enum { kFiltGeneric = 0, kFiltMfma = 1 };
enum { kFiltAuto = 0, kFiltForceGeneric = 1, kFiltForceMfma = 2 };

// The matrix kernel is the default from this many taps on, where it can serve.  profiles/filter_rates.txt (MI355X, 26e6 int8 samples):
// it is the faster of the two at every measured row, 1.4 to 1.9 times at 17 taps and 3.0 to 6.0 times at 65 and 129, its time nearly
// flat in the taps where the generic kernel's grows with them.  Below 17 taps nothing was measured and the generic kernel stays.
constexpr int kFiltMfmaMinTaps = 17;

struct FilterPlan {
    bool     launch = false;           // false: no output, nothing is launched
    int      kernel = kFiltGeneric;
    int      nout = 0, next_phase = 0;
    unsigned grid = 0, threads = 0;
    int      run = 0;                  // outputs of a workgroup's run
    int      steps = 0;                // matrix kernel: k-steps of a tile
    uint64_t runs = 0;                 // runs of the launch: workgroup w takes runs w, w + grid, ...
    size_t   lds = 0;                  // dynamic LDS of the launch, bytes
};

// whether the matrix kernel can serve: an int8 input and every tap inside two signed bytes (max_tap: the largest tap)
inline bool filter_mfma_serves(int in_size, int max_tap) { return in_size == 1 && max_tap <= kFiltMfmaMaxTap; }

// arguments in range (the caller has checked them); force: kFiltAuto, or the path GPSIQ_FILTER_KERNEL names -- taken where it can serve
inline FilterPlan plan_filter(int nsamp, int in_size, int ntaps, int decim, int phase, int max_tap, int force)
{
    FilterPlan p;
    filter_span(nsamp, decim, phase, &p.nout, &p.next_phase);
    if (p.nout <= 0) return p;
    const bool can = filter_mfma_serves(in_size, max_tap);
    const bool mfma = force == kFiltForceGeneric ? false : force == kFiltForceMfma ? can : can && ntaps >= kFiltMfmaMinTaps;
    p.launch = true;
    p.threads = kFiltThreads;
    if (mfma) {
        p.kernel = kFiltMfma;
        p.steps = filter_mfma_steps(ntaps, decim);
        p.run = filter_mfma_run(ntaps, decim);
        p.lds = (size_t) filter_mfma_plane_bytes(p.steps) + (size_t) filter_mfma_window_bytes(p.run, decim, p.steps);
    } else {
        p.run = filter_generic_run(ntaps, decim);
        p.lds = 4 * ((size_t) (p.run - 1) * (size_t) decim + (size_t) ntaps) + 4 * (size_t) ntaps;
    }
    p.runs = ((uint64_t) p.nout + (uint64_t) p.run - 1) / (uint64_t) p.run;
    p.grid = p.runs < kFiltMaxGrid ? (unsigned) p.runs : kFiltMaxGrid;
    return p;
}

// The two digit planes of the matrix kernel in fragment order (gpsiq_filter_geometry.h): lane l = (row i = l & 15, group g = l >> 4) of
// k-step t holds bytes j = 0..15, k = 64 t + 16 g + j, of A(i, k) = T[2 jj decim + c + 2 (ntaps - 1) - k], i = 2 jj + c, T the taps
// zero-stuffed.  planes: [2][steps * 1024] bytes.  cfilter_build_planes (gpsiq_cfilter_plan.h) is its complex counterpart
inline void filter_build_planes(const int16_t *taps, int ntaps, int decim, int steps, int8_t *planes)
{
    const size_t plane = (size_t) steps * kFiltK * 16;
    std::memset(planes, 0, 2 * plane);
    for (int i = 0; i < 16; ++i) {
        const int jj = i >> 1, comp = i & 1;
        for (int tap = 0; tap < ntaps; ++tap) {
            const int kk = 2 * jj * decim + comp + 2 * (ntaps - 1) - 2 * tap;      // the k at which this row meets taps[tap]
            const int t = kk / kFiltK, g = (kk % kFiltK) / 16, j = kk % 16;
            const size_t at = ((size_t) t * 64 + (size_t) (16 * g + i)) * 16 + (size_t) j;
            const int d0 = ((taps[tap] + 128) & 255) - 128, d1 = (taps[tap] - d0) / 256;
            planes[at] = (int8_t) d0;
            planes[plane + at] = (int8_t) d1;
        }
    }
}

// Blocks per piece of gpsiq_generate_batch_filtered: the one policy, stage_piece_blocks (gpsiq_pieces.h), under the call's name.  A
// piece is one span of the filter: its samples fit an int
inline int filter_piece_blocks(int nblocks, int nsamp, size_t src_block_bytes, long override_blocks) { return stage_piece_blocks(nblocks, nsamp, src_block_bytes, override_blocks); }

}  // namespace gpsiq
#endif
