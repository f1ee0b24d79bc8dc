// gpsiq_mix_plan.h -- the kernel and the grid a gpsiq_mix call (include/gpsiq_rows.h, "Mix") takes.  Host code only, and pure: no HIP,
// no environment (the GPSIQ_MIX_KERNEL override is an argument, read per call by the caller; so is GPSIQ_MIX_PIECE_BLOCKS, for the
// piece size of gpsiq_generate_batch_mixed: stage_piece_blocks, gpsiq_pieces.h).  tests/mix_plan.cpp pins every plan on the CPU.
// Not a device source: the geometry the kernels are compiled for is gpsiq_mix_geometry.h.
#ifndef GPSIQ_MIX_PLAN_H
#define GPSIQ_MIX_PLAN_H

#include <cstddef>
#include <cstdint>

#include "gpsiq_mix_geometry.h"
#include "gpsiq_pieces.h"

namespace gpsiq {

enum { kMixGeneric = 0, kMixRows = 1 };
enum { kMixAuto = 0, kMixForceGeneric = 1, kMixForceRows = 2 };

// Whether the row kernel is the default where it can serve.  profiles/mix_rates.txt (MI355X, one span of 64e6 samples, median
// kernel_ms of nine calls, the two kernels alternating in one run): it is the faster of the two at every measured shape -- 0.79 of
// the generic kernel's time for a stream plus a tone in place in int8, 0.76 in int16, 0.69 for a stream, a delayed rotated copy and
// two tones, 0.64 for eight terms -- so it is the default for every call it can serve.  Nothing else was measured.
constexpr bool kMixRowsDefault = true;

struct MixPlan {
    bool     launch = false;           // false: no sample, nothing is launched
    int      kernel = kMixGeneric;
    unsigned grid = 0, threads = 0;
    int      lead = 0;                 // row kernel: samples of the first slot that lie before sample 0 of dst
    uint64_t units = 0;                // generic: samples; row kernel: slots.  Thread t of the launch takes units t, t + grid * threads, ...
};

// Whether the row kernel can serve.  It steps the gate and the sweep position from one sample to the next instead of reducing
// m + offset anew, which is the contract's value as long as neither m nor m + offset wraps mod 2^64 inside the span: nsamp < 2^31
// and an offset < 2^32, so an m0 below 2^63 is far inside.  A span further on goes to the generic kernel, which reduces per sample.
inline bool mix_rows_serves(uint64_t m0) { return m0 < ((uint64_t) 1 << 63); }

// arguments in range (the caller has checked them); dst_addr: the destination's address (its low four bits decide the slots);
// force: kMixAuto, or the path GPSIQ_MIX_KERNEL names -- taken where it can serve
inline MixPlan plan_mix(int nsamp, uint64_t m0, int out_size, uint64_t dst_addr, int force)
{
    MixPlan p;
    if (nsamp <= 0) return p;
    const bool can = mix_rows_serves(m0);
    const bool rows = force == kMixForceGeneric ? false : force == kMixForceRows ? can : can && kMixRowsDefault;
    p.launch = true;
    p.threads = kMixThreads;
    if (rows) {
        p.kernel = kMixRows;
        p.lead = mix_lead(dst_addr, out_size);
        const uint64_t per = (uint64_t) mix_slot_samples(out_size);
        p.units = ((uint64_t) nsamp + (uint64_t) p.lead + per - 1) / per;
    } else {
        p.units = (uint64_t) nsamp;
    }
    const uint64_t wgs = (p.units + kMixThreads - 1) / kMixThreads;
    p.grid = wgs < kMixMaxGrid ? (unsigned) wgs : kMixMaxGrid;
    return p;
}

// Blocks per piece of gpsiq_generate_batch_mixed: the one policy, stage_piece_blocks (gpsiq_pieces.h), under the call's name.  A piece
// is one span of the mixer: its samples fit an int
inline int mix_piece_blocks(int nblocks, int nsamp, size_t block_bytes, long override_blocks) { return stage_piece_blocks(nblocks, nsamp, block_bytes, override_blocks); }

}  // namespace gpsiq
#endif
