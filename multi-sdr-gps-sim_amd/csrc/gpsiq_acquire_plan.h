// gpsiq_acquire_plan.h -- which kernels a gpsiq_acquire call (include/gpsiq_rows.h, "Acquisition") takes, with which grids and how
// much scratch.  Host code only, and pure: no HIP, no environment (the knob is an argument).  tests/acquire_plan.cpp pins every plan
// on the CPU.  Not a device source: the geometry the kernels are compiled for is gpsiq_acquire_geometry.h, the list of kernels that
// exist is in gpsiq_acquire_kernels.hip.  Every size is 64-bit arithmetic: nshift and nsamp go up to INT_MAX.
#ifndef GPSIQ_ACQUIRE_PLAN_H
#define GPSIQ_ACQUIRE_PLAN_H

#include <cstdint>

#include "gpsiq_acquire_geometry.h"
#include "gpsiq_launch_plan.h"

namespace gpsiq {

enum AcquireKernel { kAcquireGeneric = 0, kAcquireMfma = 1 };

inline const char *acquire_kernel_name(int k) { return k == kAcquireMfma ? "mfma" : "generic"; }

constexpr int kAcqMaxNcoh = 1 << 20, kAcqMaxDopp = 1024, kAcqMaxPrn = 32;
// whether the matrix path is the default where it can serve: decided by measurement at the workload's own shape
constexpr bool kAcqFastDefault = true;

struct AcquirePlan {
    int      kind = kPlanNothing;      // kPlanNothing: the arguments are not a search (nothing is launched) | kPlanLaunch
    int      kernel = kAcquireGeneric;
    int      digits = 0;               // mfma: balanced base-256 digits of a wiped sample (3 for int8, 4 for int16); generic: 0
    uint64_t span = 0;                 // samples the search reads: (nshift - 1) + (nnoncoh - 1) * hop + ncoh
    uint64_t cells = 0;                // nprn * ndopp * nshift: the power grid
    uint64_t corr_cells = 0;           // cells * nnoncoh
    // generic: a lane owns a shift, grid (shift blocks, bins, satellites)
    unsigned gx = 0, gy = 0, gz = 0;
    // mfma: stage one writes `row_tiles` tiles of 16 digit rows, each `npad` bytes long; stage two runs k-steps of 64 samples
    int      row_tiles = 0;
    uint64_t npad = 0, scratch_bytes = 0;
    uint64_t wipe_grid = 0;            // workgroups of acquire_wipe: one thread per (row tile, bin of it, four samples)
    unsigned mx = 0, my = 0, mz = 0;   // acquire_mfma: (blocks of 256 shifts, groups of four row tiles, satellites)
    int      ksteps = 0;
    unsigned lds_bytes = 0;            // the 16 code copies
    uint64_t peak_grid = 0;            // acquire_peaks: one wave per (satellite, bin)
};

// what the call itself checks (GPSIQ_E_ARG otherwise); the planner answers kPlanNothing for anything else
inline bool acquire_args_ok(int64_t nsamp, int sample_size, int nprn, int ndopp, int64_t nshift, int64_t ncoh, int64_t nnoncoh, int64_t hop)
{
    if (sample_size != 1 && sample_size != 2) return false;
    if (nsamp < 0 || nprn < 1 || nprn > kAcqMaxPrn || ndopp < 1 || ndopp > kAcqMaxDopp) return false;
    if (ncoh < 64 || ncoh > kAcqMaxNcoh || (ncoh & 63) || nshift < 1 || nnoncoh < 1 || hop < 1) return false;
    if (nshift > INT32_MAX || nnoncoh > INT32_MAX || hop > INT32_MAX || nsamp > INT32_MAX) return false;
    // (nshift - 1) + (nnoncoh - 1) * hop + ncoh <= nsamp, without leaving 64 bits: every factor is below 2^31
    return (nshift - 1) + (nnoncoh - 1) * hop + ncoh <= nsamp;
}

// The matrix path CAN serve any search whose code copies fit the kernel's LDS (ncoh <= kAcqMaxFastNcoh) and whose digit planes fit
// kAcqScratchCap; it is TAKEN by default (fast_default) where the search also fills at least one tile in every direction -- two bins
// (16 digit rows), 256 shifts (a wave's 16 tiles), and ncoh >= 64 always holds -- since below that most of every product is padding.
// force_generic (GPSIQ_ACQUIRE_KERNEL=generic): the generic kernel whatever the shape, the cross-check.  force_mfma (=mfma): the matrix
// path wherever it can serve, also below a full tile: the tests' way to its edges, and the way in while it is not the default.
inline AcquirePlan plan_acquire(int64_t nsamp, int sample_size, int nprn, int ndopp, int64_t nshift, int64_t ncoh, int64_t nnoncoh, int64_t hop,
                                bool force_generic, bool fast_default = kAcqFastDefault, bool force_mfma = false)
{
    AcquirePlan p;
    if (!acquire_args_ok(nsamp, sample_size, nprn, ndopp, nshift, ncoh, nnoncoh, hop)) return p;
    p.kind = kPlanLaunch;
    p.span = (uint64_t) ((nshift - 1) + (nnoncoh - 1) * hop + ncoh);
    p.cells = (uint64_t) nprn * (uint64_t) ndopp * (uint64_t) nshift;
    p.corr_cells = p.cells * (uint64_t) nnoncoh;                         // < 2^5 * 2^10 * 2^31 * 2^31: fits
    p.gx = (unsigned) ((nshift + kAcqThreads - 1) / kAcqThreads);
    p.gy = (unsigned) ndopp;
    p.gz = (unsigned) nprn;
    p.peak_grid = ((uint64_t) nprn * (uint64_t) ndopp + (kAcqThreads / 64) - 1) / (kAcqThreads / 64);

    const uint64_t s0_max = (uint64_t) ((nshift - 1) / kAcqBlockShifts) * kAcqBlockShifts;
    const uint64_t h16_max = (uint64_t) ((nnoncoh - 1) * hop) & ~UINT64_C(15);
    const uint64_t npad = s0_max + h16_max + (uint64_t) ncoh + kAcqPlaneTail;
    const int row_tiles = (ndopp + kAcqBinsPerTile - 1) / kAcqBinsPerTile;
    const uint64_t scratch = (uint64_t) row_tiles * kAcqTileRows * npad;
    const bool can = ncoh <= kAcqMaxFastNcoh && scratch <= kAcqScratchCap;
    const bool full_tile = nshift >= kAcqBlockShifts && ndopp >= kAcqBinsPerTile;
    if (force_generic || !can || !(force_mfma || (fast_default && full_tile))) return p;
    p.kernel = kAcquireMfma;
    p.digits = sample_size == 1 ? 3 : 4;
    p.row_tiles = row_tiles;
    p.npad = npad;
    p.scratch_bytes = scratch;
    p.wipe_grid = ((uint64_t) row_tiles * kAcqBinsPerTile * (npad / 4) + kAcqThreads - 1) / kAcqThreads;      // <= 2^28 / 2^9 under the cap
    p.mx = (unsigned) ((nshift + kAcqBlockShifts - 1) / kAcqBlockShifts);
    p.my = (unsigned) ((row_tiles + kAcqWaves - 1) / kAcqWaves);
    p.mz = (unsigned) nprn;
    p.ksteps = (int) (ncoh / kAcqK) + 5;
    p.lds_bytes = 16u * ((unsigned) ncoh + (unsigned) kAcqCopyPad);
    return p;
}

}  // namespace gpsiq
#endif
