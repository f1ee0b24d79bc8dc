// gpsiq_mix_geometry.h -- the geometry the mix kernels (gpsiq_mix_kernels.hip) are compiled for and the planner (gpsiq_mix_plan.h)
// cuts its grids by, and the terms as the kernels take them.  These decide device code, so the file is one of the device sources
// behind gpsiq_kernels_id() (DEVSRC of the Makefile).  Plain constants and one plain struct: host and device code include it alike.
#ifndef GPSIQ_MIX_GEOMETRY_H
#define GPSIQ_MIX_GEOMETRY_H

#include <cstdint>

namespace gpsiq {

constexpr int kMixMaxTerms = 8, kMixMaxShift = 40;
constexpr int kMixThreads = 256;
// workgroups of a launch at most: sixteen for each of the 256 CUs; a workgroup strides over the units of the launch past that and
// builds its 2 KiB table once
constexpr unsigned kMixMaxGrid = 4096;

// mix_generic: a UNIT is one complex sample, a thread takes units tid, tid + threads of the launch, ...
// mix_rows: a UNIT is a SLOT, the 16 bytes of dst at a 16-byte aligned address: kMixSlotBytes / (2 * out_sample_size) samples, fewer
// in the first and the last slot of a span whose ends are not aligned (dst is 4-byte aligned and no more: the first slot then starts
// `lead` samples before sample 0).  A lane owns a slot: it reads the in-place term's 16 bytes and later writes the same 16 bytes.
constexpr int kMixSlotBytes = 16;
constexpr int mix_slot_samples(int out_size) { return kMixSlotBytes / (2 * out_size); }
// samples of the first slot that lie before sample 0 of dst
inline int mix_lead(uint64_t dst_addr, int out_size) { return (int) (dst_addr & (kMixSlotBytes - 1)) / (2 * out_size); }

// A term as the kernels read it (gpsiq_mix_term_t of include/gpsiq_rows.h without its reserved fields), and the terms of a launch:
// a kernel argument, so they cross to the device with the launch, on its stream.
struct MixDevTerm {
    const uint8_t *src;
    uint64_t skip, phase0, step, rate;
    uint32_t sweep_period, sweep_offset, gate_period, gate_on, gate_offset;
    int32_t  gain, kind, fmt;
};
struct MixDevTerms {
    MixDevTerm t[kMixMaxTerms];
    int32_t n;
};

}  // namespace gpsiq
#endif
