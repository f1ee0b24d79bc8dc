// gpsiq_stage_call.h -- what the host side of a stream stage's call does around its kernel, stated once: the counter of clamped
// elements with its way back and the two timing events (gpsiq_pack, gpsiq_filter, gpsiq_cfilter, gpsiq_mix, gpsiq_resample), the
// argument checks the span stages word alike, the two refusals every staged batch call makes, and the GPSIQ_<STAGE>_KERNEL override.
// Host code, not a device source.  gpsiq_ctx.h includes this header ahead of the stage headers, whose sets hold a ClipCount.
// Every text below is the one the calls had each for themselves: callers and tests read them.
#ifndef GPSIQ_STAGE_CALL_H
#define GPSIQ_STAGE_CALL_H

#include <cstdlib>
#include <cstring>

#include "gpsiq_internal.h"
#include "gpsiq_own.h"

namespace gpsiq {

// the counter of clamped elements on the device and page-locked on its way back, and the two events a kernel is timed with
struct ClipCount {
    DevBuf<unsigned long long>    d_count;   PinnedBuf<unsigned long long> h_count;       // [1]
    Event          t0, t1;
    int reserve();                                  // first use
};

inline int ClipCount::reserve()
{
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(d_count.reserve(1));
    HIP_TRY(h_count.reserve(1));
    return GPSIQ_OK;
}

// A call's kernel on s with its count and its time: the counter zeroed (the workgroups add into it), t0, what `queue` queues, t1, the
// counter's way back, and the call synchronised.  queue() returns GPSIQ_OK or the code of the error it has reported: the call then
// ends at once.  What a call queues ahead of its kernel (coefficients, tables) is its own, in front of this.
template <typename Queue>
int counted_call(ClipCount &k, hipStream_t s, Queue &&queue, uint64_t *clipped, float *kernel_ms)
{
    HIP_TRY(hipMemsetAsync(k.d_count.get(), 0, sizeof(unsigned long long), s));
    HIP_TRY(hipEventRecord(k.t0.get(), s));
    if (int rc = queue()) return rc;
    HIP_TRY(hipEventRecord(k.t1.get(), s));
    HIP_TRY(hipMemcpyAsync(k.h_count.get(), k.d_count.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (clipped) *clipped = (uint64_t) k.h_count[0];
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.t0.get(), k.t1.get()));
    return GPSIQ_OK;
}

inline int check_formats(int sample_size, int out_sample_size)
{
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    if (out_sample_size != GPSIQ_SC08 && out_sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad output sample size %d", out_sample_size);
    return GPSIQ_OK;
}

// a span of nsamp samples at src with the ntaps - 1 samples before it at head (may be null), nout outputs at dst: pointers where
// there is something to read or write, 4-byte aligned, the destination apart from both sources
inline int check_span(const void *src, int nsamp, int sample_size, const void *head, int ntaps, const void *dst, uint64_t nout, int out_sample_size)
{
    if (!src && nsamp) return fail(GPSIQ_E_ARG, "null source");
    if (!dst && nout) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    if ((uintptr_t) head & 3) return fail(GPSIQ_E_ARG, "head %p not 4-byte aligned", head);
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    const size_t src_len = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, head_len = head ? (size_t) 2 * (size_t) (ntaps - 1) * (size_t) sample_size : 0;
    const size_t dst_len = (size_t) 2 * (size_t) nout * (size_t) out_sample_size;
    if (overlap(dst, dst_len, src, src_len)) return fail(GPSIQ_E_ARG, "source [%p, +%zu) and destination [%p, +%zu) overlap", src, src_len, dst, dst_len);
    if (overlap(dst, dst_len, head, head_len)) return fail(GPSIQ_E_ARG, "head [%p, +%zu) and destination [%p, +%zu) overlap", head, head_len, dst, dst_len);
    return GPSIQ_OK;
}

inline int check_batch_shape(int nblocks, int nchan, int nsamp, double fs)
{
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    if (nsamp < 0 || !(fs > 0.0)) return fail(GPSIQ_E_ARG, "bad nsamp %d / fs %g", nsamp, fs);
    return GPSIQ_OK;
}

// what the environment variable env_name asks of a stage's planner: 0 (unset, or any other word: the planner decides), 1 for
// "generic", 2 for second_word ("mfma" or "rows").  Every stage's k..Auto / k..ForceGeneric / k..Force<second> are these values
// (each static_asserts it).  Read per call
inline int forced_kernel(const char *env_name, const char *second_word)
{
    const char *env = std::getenv(env_name);
    if (!env) return 0;
    return !std::strcmp(env, "generic") ? 1 : !std::strcmp(env, second_word) ? 2 : 0;
}

}  // namespace gpsiq
#endif
