// gpsiq_launch_plan.h -- which synthesis kernel renders a set of blocks, and with which grid.  Host code only, and pure: no HIP,
// and every environment value is an argument (seg_policy_from_env() alone reads the GPSIQ_SEG_* / GPSIQ_NO_FAST variables; the
// launcher, gpsiq_launch.cpp, calls it once per process).  tests/launch_plans.cpp pins every plan on the CPU.  Not a device
// source: the geometry the kernels are compiled for is gpsiq_geometry.h, the list of kernels that exist is in gpsiq_kernels.hip.
#ifndef GPSIQ_PLAN_SYNTH_H
#define GPSIQ_PLAN_SYNTH_H

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/gpsiq.h"
#include "gpsiq_geometry.h"

namespace gpsiq {

// Kernel variants (gpsiq_launch's `variant`).
enum Variant {
    kAuto = 0,      // fast when every resident descriptor allows it, else generic
    kGeneric = 1,   // one sample per thread, full-width closed form per sample (any rate)
    kRows = 2,      // 64-sample rows per wave, incremental NCOs, LDS-staged windows
    kRowsX = 3,     // same rows, channel-inner loop order with all NCO state in registers
    kTile = 4,      // rowsx with trimmed per-tile overhead, 64 rows per wave (32768-sample tiles)
    kSeg = 5,       // tile kernel, each wave running several consecutive 64-row chunks
    kSegHalf = 6,   // seg with one window per 32 samples: for sample rates down to 1.023 Msps
    kSegMask = 7,   // high sample rates: per-(channel,row) 64-bit sign masks from a pre-pass, applied as EXEC masks
    kSegBoth = 8,   // seg's plain-add core with a both-polarity LUT (sign concatenated above the index), 16-wave workgroups
    kNumVariants
};

inline const char *variant_name(int v)
{
    switch (v) {
    case kAuto: return "auto";
    case kGeneric: return "generic";
    case kRows: return "rows";
    case kRowsX: return "rowsx";
    case kTile: return "tile";
    case kSeg: return "seg";
    case kSegHalf: return "segh";
    case kSegMask: return "segm";
    case kSegBoth: return "segb";
    default: return "?";
    }
}

// receiver noise and the output level exist in the default kernels (seg, segh, generic) and tile
inline bool has_noise_path(int v) { return v == kGeneric || v == kTile || v == kSeg || v == kSegHalf; }

// The row kernel needs all 64 lanes of a row inside one 32-chip window:
// 63*code_step + (1 chip) <= 32 chips.
constexpr uint64_t kRowsMaxCodeStep = ((UINT64_C(31) << GPSIQ_CODE_FRAC_BITS) - 1) / 63;
// With a window per half row (32 lanes): 31*code_step + (1 chip) <= 32 chips, i.e. up to one
// chip per sample (fs >= 1.023 Msps).
constexpr uint64_t kHalfRowsMaxCodeStep = ((UINT64_C(31) << GPSIQ_CODE_FRAC_BITS) - 1) / 31;

// what kAuto means for descriptors whose largest code step is max_code_step
inline int auto_variant(uint64_t max_code_step)
{
    return max_code_step <= kRowsMaxCodeStep ? kSeg : max_code_step <= kHalfRowsMaxCodeStep ? kSegHalf : kGeneric;
}

// What a set of descriptors contributes to the choice of kernel.
struct SynthClass {
    uint64_t max_code_step = 0;     // largest code step of any channel
    int      max_active = 0;        // most active channels in any block
    long     max_amplitude = 0;     // largest sum over a block's channels of (int)(250*|gain|): bound on |I|, |Q|
};

// Noise and level as far as they bear on the choice (noise::Launch: tab set, max_z, mult set).
struct StageState {
    bool table = false;             // a noise table is given (the noise is on, or the level is and draws zeros)
    long max_z = 0;                 // max |z| while the noise is on, else 0
    bool level = false;
};

// Grid-shape policy of the seg variants; the defaults can be overridden for experiments with
// GPSIQ_SEG_TAIL_WGS / GPSIQ_SEG_MAX_WAVE_ROWS / GPSIQ_SEG_SETUP_ROWS / GPSIQ_SEG_DRAIN.
struct SegPolicy {
    int    tail_wgs = 512;          // one-chunk workgroups at the end of the grid
    int    max_wave_rows = 512;     // longest run of rows a wave may own
    double setup_rows = 3.5;        // per-workgroup set-up, in row-times (measured: tile vs seg = 4 %)
    double drain_rounds = 0.3;      // time lost while the grid drains, in workgroup durations
    double resident_wgs = 512.0;    // 256 CUs x 2 workgroups (67 KB LDS each)
    bool   allow_fast = true;       // GPSIQ_NO_FAST=1 forces the packed-multiply kernels (A/B experiments, tests)
};

inline SegPolicy seg_policy_from_env()
{
    SegPolicy p;
    if (const char *e = std::getenv("GPSIQ_SEG_TAIL_WGS")) p.tail_wgs = std::atoi(e);
    if (const char *e = std::getenv("GPSIQ_SEG_MAX_WAVE_ROWS")) p.max_wave_rows = std::atoi(e);
    if (const char *e = std::getenv("GPSIQ_SEG_SETUP_ROWS")) p.setup_rows = std::atof(e);
    if (const char *e = std::getenv("GPSIQ_SEG_DRAIN")) p.drain_rounds = std::atof(e);
    if (const char *e = std::getenv("GPSIQ_NO_FAST")) p.allow_fast = std::atoi(e) == 0;
    return p;
}

// scratch a launch of `variant` needs (segm: one 64-bit mask per channel slot and row)
inline size_t variant_scratch_bytes(int variant, int nsamp, int nblocks)
{
    if (variant != kSegMask || nsamp <= 0 || nblocks <= 0) return 0;
    return (size_t) nblocks * (size_t) ((nsamp + 63) / 64) * 16u * sizeof(uint64_t);
}

enum PlanKind { kPlanNothing, kPlanNoPath, kPlanLaunch };     // no samples to render | noise or level on a variant without them
enum Family { kPlain, kNoise, kLevel };                      // synth_tile, synth_tile_noise, synth_tile_level

// Everything the launcher needs to know about one launch.
struct SynthPlan {
    int      kind = kPlanNothing;
    int      variant = kGeneric;    // after the fall-backs (never kAuto)
    int      family = kPlain;
    int      slots = 0, rows = 0, H = 1;    // template arguments: channel slots, rows per chunk, windows per row
    bool     fast = false;          // the plain-add core
    unsigned grid = 0, threads = 0;
    // the kernels' shape arguments
    int      tiles = 0;             // workgroups per block (of the big workgroups, where there is a tail)
    int      wave_rows = 0, big_wgs = 0, big_blocks = 0, tiles_small = 0;     // tile / seg / segh / segb
    unsigned pre_grid = 0;          // segm: the grid of sign_masks (kMaskThreads threads each) ...
    int      rows_total = 0, rowgroups = 0;
    int      tile_samples = 0;      // generic
};

inline SynthPlan plan_synth(int variant, int nsamp, int nblocks, int sample_size, const SynthClass &cls, bool have_scratch,
                            const StageState &st, const SegPolicy &pol)
{
    SynthPlan p;
    if (nblocks <= 0 || nsamp <= 0) return p;
    if ((st.table || st.level) && !has_noise_path(variant)) { p.kind = kPlanNoPath; return p; }
    p.kind = kPlanLaunch;
    // no channel sum of any resident block can leave the int16 range: plain-add kernel
    // (the int8 kernels keep 12-bit fields and are exact for any gain)
    // (with noise the bound is on |I + zI|: max_amplitude + max|z|; with the output level the noise is added outside the packed
    // word and both formats run the int16 cores: the bound is on the signal alone)
    p.fast = (st.level ? cls.max_amplitude <= 32767 : sample_size == GPSIQ_SC08 || cls.max_amplitude + st.max_z <= 32767) && pol.allow_fast;
    // the mask kernel only has the plain-add LUT formats: int16 sums that may leave the int16 range go to seg's packed core
    if (variant == kSegMask && ((sample_size == GPSIQ_SC16 && cls.max_amplitude > 32767) || !have_scratch)) variant = kSeg;
    // the both-polarity table is a form of the plain-add core: sums that may leave the int16 range go to seg's packed core
    if (variant == kSegBoth && !p.fast) variant = kSeg;
    if (variant < kRows || variant > kSegBoth) variant = kGeneric;
    p.variant = variant;
    p.family = st.level ? kLevel : st.table ? kNoise : kPlain;
    p.slots = cls.max_active <= 4 ? 4 : cls.max_active <= 8 ? 8 : cls.max_active <= 12 ? 12 : 16;
    if (variant == kRowsX && p.slots == 12) p.slots = 16;
    p.threads = variant == kGeneric ? kGenericThreads : kRowsThreads;
    p.rows_total = (nsamp + 63) / 64;

    if (variant == kGeneric) {
        p.tile_samples = 4096;
        p.tiles = (nsamp + p.tile_samples - 1) / p.tile_samples;
        p.grid = (unsigned) (p.tiles * nblocks);
    } else if (variant == kRows || variant == kRowsX) {
        p.tiles = (nsamp + kRowsTile - 1) / kRowsTile;
        p.grid = (unsigned) (p.tiles * nblocks);
    } else if (variant == kSegMask) {
        p.rowgroups = (p.rows_total + kMaskRowsPerThread - 1) / kMaskRowsPerThread;
        const size_t threads = (size_t) nblocks * p.rowgroups * 16;
        p.pre_grid = (unsigned) ((threads + kMaskThreads - 1) / kMaskThreads);
        // every wave the same number of rows; workgroups of ~256 rows per wave amortise the LUT build
        p.tiles = (p.rows_total + kWaves * 256 - 1) / (kWaves * 256);
        p.wave_rows = (p.rows_total + kWaves * p.tiles - 1) / (kWaves * p.tiles);
        p.grid = (unsigned) (p.tiles * nblocks);
    } else {
        p.H = variant == kSegHalf ? 2 : 1;
        // rows per chunk (the window array of tile / seg / segh holds 64 windows per wave)
        p.rows = variant == kSegBoth ? both_rows(p.slots) : 64 / p.H;
        // seg: many rows per wave amortise the per-workgroup set-up (LUT build, start products),
        // but long workgroups make the drain of the grid expensive.  Every block is cut into
        // nwg workgroups whose 8 waves all get the same number of rows, so no wave idles while
        // its workgroup holds a CU slot, whatever the block length.  nwg maximises
        //   (rows used / rows scheduled) x (rows per wave / (rows per wave + set-up)) x (rounds / (rounds + drain)),
        // a model fitted to the measured variant sweeps; the last blocks are covered by
        // one-chunk workgroups so that the drain is short.  (tile: one chunk per wave throughout.)
        const int rows = p.rows, rows_total = p.rows_total;
        const int tiles1 = (rows_total + kWaves * rows - 1) / (kWaves * rows);
        int tail_blocks = 0;
        p.wave_rows = rows;
        p.tiles = tiles1;
        if (variant != kTile) {
            double best = 0.0;
            for (int nwg = 1; nwg <= tiles1; ++nwg) {
                const int wr = (rows_total + kWaves * nwg - 1) / (kWaves * nwg);
                if (wr > pol.max_wave_rows) continue;
                if (wr < rows && nwg < tiles1) break;
                const double fill = (double) rows_total / ((double) kWaves * nwg * wr);
                const double amort = (double) wr / ((double) wr + pol.setup_rows);
                const double rounds = (double) nblocks * nwg / pol.resident_wgs;
                const double score = fill * amort * rounds / (rounds + pol.drain_rounds);
                if (score > best) { best = score; p.wave_rows = wr > rows ? wr : rows; p.tiles = nwg; }
            }
            if (p.wave_rows > rows) {
                tail_blocks = (pol.tail_wgs + tiles1 - 1) / tiles1;
                if (tail_blocks > nblocks / 2) tail_blocks = nblocks / 2;
            }
        }
        p.tiles_small = tiles1;
        p.big_blocks = nblocks - tail_blocks;
        p.big_wgs = p.tiles * p.big_blocks;
        p.grid = (unsigned) (p.big_wgs + tiles1 * tail_blocks);
    }
    return p;
}

}  // namespace gpsiq
#endif
