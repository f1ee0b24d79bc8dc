// gpsiq_agc.h -- what the device context holds for gpsiq_agc / gpsiq_generate_batch_agc (include/gpsiq_rows.h, "AGC") and what their
// host side (gpsiq_agc.cpp) and their kernels (gpsiq_agc_kernels.hip, with gpsiq_agc_geometry.h) use of each other.  The plan is in
// gpsiq_agc_plan.h.  Host code; gpsiq_ctx.h includes this header for the context's member `agc`.
#ifndef GPSIQ_AGC_H
#define GPSIQ_AGC_H

#include "gpsiq_internal.h"
#include "gpsiq_own.h"
#include "gpsiq_agc_geometry.h"

namespace gpsiq {

// What a call keeps on the device besides its scratch: both counts and the state twice.  A launch reads st[k] and writes st[k ^ 1]
// (agc_gains gives one thread per window the ring as it was, so the ring it leaves is another one); the pieces of a batch call take
// the two in turn, and the whole block comes back once, behind the last launch.  The counts lead, 64 bits each: the piece loop of the
// staged batch calls fetches them as its counter (gpsiq_stage_batch.h, count_words)
struct AgcBack {
    unsigned long long clipped, blanked;
    gpsiq_agc_state_t  st[2];
};
static_assert(sizeof(AgcBack) % sizeof(unsigned long long) == 0, "AgcBack comes back as 64-bit words");

// the gain rule's share of a configuration, as the gains kernel takes it by value
struct AgcGain { uint32_t target_q8, mult0, mult_min, mult_max; int32_t navg; };

// the block above on the device and its page-locked twin, the scratch of a launch (per window a sum, a count and a multiplier, and the
// blank mask: gpsiq_agc_plan.h), and the events gpsiq_agc times its launches with: before the first, and behind each of the three.
// The batch call works through its pieces with the context's staging ring (gpsiq_stage_batch.h)
struct AgcSet {
    DevBuf<AgcBack>    d_back;    PinnedBuf<AgcBack> h_back;         // [1]
    DevBuf<uint8_t>    d_scratch;                                    // bytes
    Event              t[4];
    long long          last[6] = {-1, 0, 0, 0, 0, 0};   // the last call's plan (gpsiq_agc_last_plan)
    float              last_ms[3] = {0.0f, 0.0f, 0.0f}; // device time of the last gpsiq_agc's three launches (gpsiq_agc_last_ms)
    int reserve(size_t scratch_bytes);                  // first use + room for one launch's scratch
};

inline int AgcSet::reserve(size_t scratch_bytes)
{
    for (auto &e : t) HIP_TRY(e.ensure(hipEventDefault));
    HIP_TRY(d_back.reserve(1));
    HIP_TRY(h_back.reserve(1));
    HIP_TRY(reserve_together(scratch_bytes, scratch_bytes + scratch_bytes / 4 + 256, d_scratch));
    return GPSIQ_OK;
}

// The kernels (gpsiq_agc_kernels.hip).
// agc_measure: span, its samples, the fill before it, the window, blank_thresh, blank_hold, the state read (hold) and the state
// written (hold, where the blanker is on), per-window sums and counts (zeroed by the host), the mask (blanker on), the count of
// blanked samples
using AgcMeasureFn = void (*)(const uint8_t *, int, uint32_t, uint32_t, int, int, const gpsiq_agc_state_t *, gpsiq_agc_state_t *, unsigned long long *,
                              uint32_t *, uint8_t *, unsigned long long *);
// agc_gains: windows touched, samples, fill, window, the gain rule, whether agc_measure has written the hold, the state read and the
// state written, sums, counts, the multipliers
using AgcGainsFn = void (*)(uint32_t, int, uint32_t, uint32_t, AgcGain, int, const gpsiq_agc_state_t *, gpsiq_agc_state_t *, const unsigned long long *,
                            const uint32_t *, uint32_t *);
// agc_apply: span, samples, fill, window, multipliers, mask (nullptr: blanker off), the state read (hold), qmax, destination, units
// of the span, the count of clamped elements
using AgcApplyFn = void (*)(const uint8_t *, int, uint32_t, uint32_t, const uint32_t *, const uint8_t *, const gpsiq_agc_state_t *, int, uint8_t *, uint32_t,
                            unsigned long long *);
AgcMeasureFn agc_measure_kernel(int in_fmt, bool mask);
AgcGainsFn   agc_gains_kernel();
AgcApplyFn   agc_apply_kernel(int in_fmt, int out_fmt, bool mask);

}  // namespace gpsiq

// gpsiq_agc.cpp: gpsiq_agc and gpsiq_generate_batch_agc themselves, behind the plumbing entries "agc" and "generate_batch_agc".
// Declared from the public prototypes, and hidden: a definition that has drifted from include/gpsiq_rows.h is another function, and
// the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_agc) gpsiq_agc_impl;
__attribute__((visibility("hidden"))) decltype(gpsiq_generate_batch_agc) gpsiq_generate_batch_agc_impl;
#endif
