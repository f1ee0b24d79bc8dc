// gpsiq_resample_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_resample (include/gpsiq_rows.h, "Resample"): a polyphase
// resampler over ONE contiguous span of interleaved I,Q samples, int8 or int16.  Output j sits at p_j = pos0 + j * step in units of
// 2^-32 input sample; its integer part picks the input window, its fraction the row of the tap table and, with interp, the weight
// between that row and the next.
//   resample_generic<IN, OUT>       every legal call: one output per thread, p_j from the closed form, samples through x(m) from
//                                   global memory, the tap table in LDS.  The kernel the other one is compared against.
//   resample_rows<IN, OUT, PAD>     the hot path: a workgroup takes a run of kRsRun consecutive outputs, stages the input window of the
//                                   run in LDS as filter_generic stages its window, and each lane accumulates whole outputs in int32
// One accumulator width, no saturation inside a sum: every row has sum |taps| <= 65535 (checked on the host, GPSIQ_E_RANGE) and
// |x| <= 32768, so |a0|, |a1| <= 65535 * 32768 < 2^31.  With interp both rows are accumulated and combined in 64 bits,
// (256 - mu) a0 + mu a1 + 2^(shift + 7) >> shift + 8; without, a0 is rounded by shift as the filter rounds.  Symmetric clamp, one flag
// per element the clamp changed.  x(m), the store of a sample and the count are gpsiq_stream.h's (sample_at, store_sample,
// count_clipped); the rounding is this stage's own arithmetic and stays here (rs_finish).
// Every offset into src / dst is 64 bits wide, and so is j: a span of 2^31 - 1 samples at step 2^29 has 2^34 outputs.  p_j itself
// stays below nsamp * 2^32 < 2^63 for every output that exists.  Sample m of the span is read only for 0 <= m < nsamp, sample m < 0
// from head (or as zero); outputs j < nout are written and nothing else.  No workgroup waits for another; a workgroup strides over
// the units of the launch.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_resample_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::sample_at;
using stream::store_sample;
using stream::count_clipped;

// the contract's y of one element from its row sums, clamped to +-QMAX; clipped counts the elements the clamp changed
template <int OUT>
__device__ __forceinline__ int rs_finish(int a0, int a1, int mu, int shift, int interp, unsigned &clipped)
{
    constexpr int QMAX = OUT == GPSIQ_SC08 ? 127 : 32767;
    int64_t y;
    if (interp) y = ((int64_t) (256 - mu) * (int64_t) a0 + (int64_t) mu * (int64_t) a1 + ((int64_t) 1 << (shift + 7))) >> (shift + 8);
    else y = ((int64_t) a0 + (shift ? (int64_t) 1 << (shift - 1) : 0)) >> shift;
    const int64_t c = y < -QMAX ? -QMAX : y > QMAX ? QMAX : y;
    clipped += c != y;
    return (int) c;
}

// the tap table of a call into LDS, rows of resample_tap_stride(ntaps) dwords (gpsiq_resample_geometry.h); the caller synchronises
__device__ __forceinline__ void rs_stage_taps(uint32_t *tap, const int16_t *__restrict__ taps, int log2_phases, int ntaps)
{
    const int ts = resample_tap_stride(ntaps), total = resample_table_dwords(log2_phases, ntaps);
    for (int i = threadIdx.x; i < total; i += kRsThreads) {
        const int r = i / ts, k = 2 * (i - r * ts);
        const uint32_t lo = k < ntaps ? (uint32_t) (uint16_t) taps[r * ntaps + k] : 0u;
        const uint32_t hi = k + 1 < ntaps ? (uint32_t) (uint16_t) taps[r * ntaps + k + 1] : 0u;
        tap[i] = lo | (hi << 16);
    }
}

// one tap against one sample, I and Q
__device__ __forceinline__ void rs_mac(int t, uint32_t v, int &ai, int &aq)
{
    ai += t * (int) (int16_t) (v & 0xffffu);
    aq += t * ((int32_t) v >> 16);
}

// row and weight of a position's fraction f: q = f >> (32 - L) (0 at L == 0), mu = interp ? (f >> (24 - L)) & 255 : 0
__device__ __forceinline__ void rs_phase(uint32_t f, int log2_phases, int interp, int &q, int &mu)
{
    q = log2_phases ? (int) (f >> (32 - log2_phases)) : 0;
    mu = interp ? (int) ((f >> (24 - log2_phases)) & 255u) : 0;
}

// Arguments: span and its samples, head (may be null), the device table int16 [nphases + 1][ntaps], log2 of the phases, ntaps, shift,
// interp, step, pos0, destination, outputs of the span, units of the launch (gpsiq_resample_plan.h), the counter (zeroed by the host).
// Dynamic LDS: the tap table.
template <int IN, int OUT>
__global__ __launch_bounds__(kRsThreads) void resample_generic(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                                const int16_t *__restrict__ taps, int log2_phases, int ntaps, int shift, int interp,
                                                                uint64_t step, uint64_t pos0, uint8_t *__restrict__ dst, uint64_t nout, uint64_t runs,
                                                                unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    uint32_t *tap = reinterpret_cast<uint32_t *>(rs_lds);
    rs_stage_taps(tap, taps, log2_phases, ntaps);
    __syncthreads();
    const int ts = resample_tap_stride(ntaps);
    unsigned clipped = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const uint64_t j = r * kRsGenericUnit + threadIdx.x;
        if (j >= nout) continue;
        const uint64_t p = pos0 + j * step;
        const int64_t m = (int64_t) (p >> 32);
        int q, mu;
        rs_phase((uint32_t) p, log2_phases, interp, q, mu);
        const uint32_t *t0 = tap + q * ts, *t1 = t0 + (interp ? ts : 0);
        int a0i = 0, a0q = 0, a1i = 0, a1q = 0;
        for (int k = 0; k < ntaps; ++k) {
            const uint32_t v = sample_at<IN>(src, head, m - k, nsamp, ntaps);
            const int sh = (k & 1) << 4;
            rs_mac((int) (int16_t) (t0[k >> 1] >> sh), v, a0i, a0q);
            if (interp) rs_mac((int) (int16_t) (t1[k >> 1] >> sh), v, a1i, a1q);
        }
        store_sample<OUT>(dst, j, rs_finish<OUT>(a0i, a1i, mu, shift, interp, clipped), rs_finish<OUT>(a0q, a1q, mu, shift, interp, clipped));
    }
    count_clipped<kRsThreads>(clipped, count);
}

// where sample i of a run's window lies (gpsiq_resample_geometry.h)
template <bool PAD>
__device__ __forceinline__ int rs_widx(int i) { return PAD ? i + (i >> 5) : i; }

// the sums of one output from the staged window: x points at x(m_j) (plain layout) or base is its index (padded)
template <bool PAD, bool INTERP>
__device__ __forceinline__ void rs_sums(const uint32_t *win, int base, const uint32_t *t0, int ts, int ntaps, int &a0i, int &a0q, int &a1i, int &a1q)
{
    const uint32_t *t1 = t0 + ts;
    int k = 0;
    for (; k + 1 < ntaps; k += 2) {
        const uint32_t v0 = win[rs_widx<PAD>(base - k)], v1 = win[rs_widx<PAD>(base - k - 1)];
        const uint32_t c0 = t0[k >> 1];
        rs_mac((int) (int16_t) (c0 & 0xffffu), v0, a0i, a0q);
        rs_mac((int32_t) c0 >> 16, v1, a0i, a0q);
        if (INTERP) {
            const uint32_t c1 = t1[k >> 1];
            rs_mac((int) (int16_t) (c1 & 0xffffu), v0, a1i, a1q);
            rs_mac((int32_t) c1 >> 16, v1, a1i, a1q);
        }
    }
    if (k < ntaps) {                                                 // an odd tap count's last
        const uint32_t v0 = win[rs_widx<PAD>(base - k)];
        rs_mac((int) (int16_t) (t0[k >> 1] & 0xffffu), v0, a0i, a0q);
        if (INTERP) rs_mac((int) (int16_t) (t1[k >> 1] & 0xffffu), v0, a1i, a1q);
    }
}

// Arguments as resample_generic's, with the outputs of a run before the runs of the launch.
// Dynamic LDS: the tap table, then the window of a run: resample_window(run, step, ntaps) samples, padded or not.
// With interp the two rows are two accumulators a lane: the sums are the contract's a0 and a1 themselves, for both input formats.
template <int IN, int OUT, bool PAD>
__global__ __launch_bounds__(kRsThreads) void resample_rows(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                             const int16_t *__restrict__ taps, int log2_phases, int ntaps, int shift, int interp,
                                                             uint64_t step, uint64_t pos0, uint8_t *__restrict__ dst, uint64_t nout, int run,
                                                             uint64_t runs, unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
    uint32_t *tap = reinterpret_cast<uint32_t *>(rs_lds);
    uint32_t *win = tap + resample_table_dwords(log2_phases, ntaps);
    const int tid = threadIdx.x, ts = resample_tap_stride(ntaps);
    rs_stage_taps(tap, taps, log2_phases, ntaps);
    unsigned clipped = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const uint64_t j0 = r * (uint64_t) run;
        const int n = nout - j0 < (uint64_t) run ? (int) (nout - j0) : run;                          // outputs of this run
        const int64_t m_first = (int64_t) ((pos0 + j0 * step) >> 32), m_last = (int64_t) ((pos0 + (j0 + (uint64_t) (n - 1)) * step) >> 32);
        const int64_t m_lo = m_first - (ntaps - 1);                                                  // the window's first sample
        const int wlen = (int) (m_last - m_lo) + 1;                                                  // its last: m_last < nsamp
        __syncthreads();                                                                             // the run before has read its window
        for (int i = tid; i < wlen; i += kRsThreads) win[rs_widx<PAD>(i)] = sample_at<IN>(src, head, m_lo + i, nsamp, ntaps);
        __syncthreads();
        for (int o = tid; o < n; o += kRsThreads) {
            const uint64_t p = pos0 + (j0 + (uint64_t) o) * step;
            const int base = (int) ((int64_t) (p >> 32) - m_lo);                                     // x(m_j), taps walk down from it
            int q, mu;
            rs_phase((uint32_t) p, log2_phases, interp, q, mu);
            int a0i = 0, a0q = 0, a1i = 0, a1q = 0;
            if (interp) rs_sums<PAD, true>(win, base, tap + q * ts, ts, ntaps, a0i, a0q, a1i, a1q);
            else rs_sums<PAD, false>(win, base, tap + q * ts, ts, ntaps, a0i, a0q, a1i, a1q);
            store_sample<OUT>(dst, j0 + (uint64_t) o, rs_finish<OUT>(a0i, a1i, mu, shift, interp, clipped),
                              rs_finish<OUT>(a0q, a1q, mu, shift, interp, clipped));
        }
    }
    count_clipped<kRsThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_resample.cpp looks up.  nullptr: no such kernel.
ResampleGenericFn resample_generic_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? resample_generic<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? resample_generic<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? resample_generic<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? resample_generic<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}

template <bool PAD>
static ResampleRowsFn rows_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? resample_rows<GPSIQ_SC08, GPSIQ_SC08, PAD> : out_fmt == GPSIQ_SC16 ? resample_rows<GPSIQ_SC08, GPSIQ_SC16, PAD> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? resample_rows<GPSIQ_SC16, GPSIQ_SC08, PAD> : out_fmt == GPSIQ_SC16 ? resample_rows<GPSIQ_SC16, GPSIQ_SC16, PAD> : nullptr;
    return nullptr;
}

ResampleRowsFn resample_rows_kernel(int in_fmt, int out_fmt, bool pad) { return pad ? rows_kernel<true>(in_fmt, out_fmt) : rows_kernel<false>(in_fmt, out_fmt); }
}  // namespace gpsiq
