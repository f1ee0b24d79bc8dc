// gpsiq_cfilter.h -- what the host side of gpsiq_cfilter (include/gpsiq_rows.h, "Complex filter and notch"; gpsiq_cfilter.cpp) and its
// kernels (gpsiq_cfilter_kernels.hip, with gpsiq_cfilter_geometry.h) use of each other.  The plan is in gpsiq_cfilter_plan.h; what the
// device context holds for the stage, its member `cfilt`, is a FirSet of its own (gpsiq_filter.h).  Host code.
#ifndef GPSIQ_CFILTER_H
#define GPSIQ_CFILTER_H

#include "gpsiq_internal.h"
#include "gpsiq_cfilter_geometry.h"

namespace gpsiq {

// the stage's kernels (gpsiq_cfilter_kernels.hip).  Arguments: span and its samples, head, the taps as dwords (generic) or the digit
// planes (matrix), ntaps, shift, decim, phase, destination, outputs of the span, outputs of a run, runs of the launch
// (gpsiq_cfilter_plan.h); matrix kernel: the k-steps of a tile and the two row constants; the counter of clamped elements.
// An int8 input's matrix kernel is filter_mfma (gpsiq_filter.h: FilterMfmaFn, filter_mfma_kernel)
using CfilterGenericFn = void (*)(const uint8_t *, int, const uint8_t *, const uint32_t *, int, int, int, int, uint8_t *, int, int, uint64_t,
                                  unsigned long long *);
using CfilterMfma16Fn  = void (*)(const uint8_t *, int, const uint8_t *, const uint8_t *, int, int, int, int, uint8_t *, int, int, uint64_t, int,
                                  int, int, unsigned long long *);
CfilterGenericFn cfilter_generic_kernel(int in_fmt, int out_fmt);
CfilterMfma16Fn  cfilter_mfma16_kernel(int out_fmt);

}  // namespace gpsiq

// gpsiq_cfilter.cpp: gpsiq_cfilter itself, behind the plumbing entry "cfilter".  Declared from the public prototype, and hidden: a
// definition that has drifted from include/gpsiq_rows.h is another function, and the library no longer links
__attribute__((visibility("hidden"))) decltype(gpsiq_cfilter) gpsiq_cfilter_impl;
#endif
