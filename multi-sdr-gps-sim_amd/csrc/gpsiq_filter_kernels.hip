// gpsiq_filter_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_filter (include/gpsiq_rows.h, "Filter"): an integer FIR over
// ONE contiguous span of interleaved I,Q samples, int8 or int16, decimated, rounded, clamped and counted.
//   filter_generic<IN, OUT>   every format pair, every legal ntaps / decim / phase: a workgroup stages the window of its run of outputs
//                             in LDS, a thread accumulates whole outputs in int32
//   filter_mfma<OUT>          int8 input: v_mfma_i32_16x16x64_i8 with the TAPS as the banded Toeplitz operand A and the stream as B
//                             (gpsiq_filter_geometry.h has the tile); the taps in two signed digit planes, recombined in int32
// One accumulator width, no saturation inside the sum: sum |taps[k]| <= 65535 (checked on the host, GPSIQ_E_RANGE) and |x| <= 32768
// give |acc| <= 65535 * 32768 = 2^31 - 32768 < 2^31 for int16 input, and |acc| <= 65535 * 128 < 2^23 for int8.  Both kernels end in
// the same finish(): round half up by `shift` (in 64 bits: acc + 2^(shift-1) may pass 2^31), symmetric clamp, one flag per element
// the clamp changed.
// Every offset into src / dst is 64 bits wide: 2^31 - 1 int16 samples are 2^33 bytes.  Sample m of the span is read only for
// 0 <= m < nsamp, sample m < 0 from head (or as zero); outputs j < nout are written and nothing else.  No workgroup waits for
// another; a workgroup strides over the runs of the launch.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_filter_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::sample_at;
using stream::finish;
using stream::store_sample;
using stream::count_clipped;

// Arguments: span and its samples, head (may be null), device taps as dwords, ntaps, shift, decim, phase, destination, outputs of the
// span, outputs of a run, runs of the launch (gpsiq_filter_plan.h), the counter (zeroed by the host).
// Dynamic LDS: [(run - 1) * decim + ntaps] window dwords, [ntaps] taps.
template <int IN, int OUT>
__global__ __launch_bounds__(kFiltThreads) void filter_generic(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                                const int32_t *__restrict__ taps, int ntaps, int shift, int decim, int phase,
                                                                uint8_t *__restrict__ dst, int nout, int run, uint64_t runs,
                                                                unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t filt_lds[];
    uint32_t *win = reinterpret_cast<uint32_t *>(filt_lds);
    int32_t *tap = reinterpret_cast<int32_t *>(filt_lds) + ((run - 1) * decim + ntaps);
    const int tid = threadIdx.x;
    for (int k = tid; k < ntaps; k += kFiltThreads) tap[k] = taps[k];
    unsigned clipped = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t j0 = (int64_t) r * run;
        const int n = (int64_t) nout - j0 < (int64_t) run ? (int) ((int64_t) nout - j0) : run;       // outputs of this run
        const int64_t m_lo = (int64_t) phase + j0 * decim - (ntaps - 1);                             // the window's first sample
        const int wlen = (n - 1) * decim + ntaps;                                                    // its last: m_j of the run's last output, < nsamp
        __syncthreads();                                                                             // the run before has read its window
        for (int i = tid; i < wlen; i += kFiltThreads) win[i] = sample_at<IN>(src, head, m_lo + i, nsamp, ntaps);
        __syncthreads();
        for (int o = tid; o < n; o += kFiltThreads) {
            const uint32_t *x = win + o * decim + (ntaps - 1);                                       // x(m_j), taps walk down from it
            int ai = 0, aq = 0;
            for (int k = 0; k < ntaps; ++k) {
                const uint32_t v = x[-k];
                const int t = tap[k];
                ai += t * (int) (int16_t) (v & 0xffffu);
                aq += t * ((int32_t) v >> 16);
            }
            store_sample<OUT>(dst, (uint64_t) (j0 + o), finish<OUT>(ai, shift, clipped), finish<OUT>(aq, shift, clipped));
        }
    }
    count_clipped<kFiltThreads>(clipped, count);
}

// Arguments as filter_generic's, with the digit planes in the taps' place and the k-steps of a tile behind the run.
// Dynamic LDS: [2][steps][64][16] plane bytes in fragment order, then the window of the run, 16-byte aligned.
// Lanes (gpsiq_acquire_kernels.hip measured the map): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds column
// l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2): lane (col, q) ends with I and Q of outputs
// 2 q and 2 q + 1 of column col.
// Digit planes: taps[k] = d0 + 256 d1, d0 = ((taps[k] + 128) & 255) - 128 in [-128, 127], d1 = (taps[k] - d0) / 256 in [-128, 127] for
// taps[k] <= 32639 (the planner sends larger taps to filter_generic).  Partial sums: |P0| <= 128 * sum |d0| <= 128 * 128 * 512 = 2^23;
// |d1| <= (|taps[k]| + 128) / 256, so sum |d1| <= (65535 + 128 * 512) / 256 < 512 and |P1| <= 128 * 512 = 2^16, |256 P1| <= 2^24:
// P0, 256 P1 and P0 + 256 P1 = acc are all inside int32, and acc is the generic kernel's to the bit.  Bytes of the window past the
// span are staged as zeros, bytes a row does not reach meet zeros of A.
template <int OUT>
__global__ __launch_bounds__(kFiltThreads) void filter_mfma(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                             const uint8_t *__restrict__ planes, int ntaps, int shift, int decim, int phase,
                                                             uint8_t *__restrict__ dst, int nout, int run, uint64_t runs, int steps,
                                                             unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t filt_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int plane_bytes = filter_mfma_plane_bytes(steps);
    uint8_t *win = filt_lds + plane_bytes;
    const int wsamp = filter_mfma_window_bytes(run, decim, steps) / 2;                               // samples staged per run
    for (int i = tid; i < plane_bytes / 16; i += kFiltThreads)
        reinterpret_cast<i32x4 *>(filt_lds)[i] = reinterpret_cast<const i32x4 *>(planes)[i];
    const int col = lane & 15, q = lane >> 4;
    unsigned clipped = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t j0 = (int64_t) r * run;
        const int n = (int64_t) nout - j0 < (int64_t) run ? (int) ((int64_t) nout - j0) : run;
        const int64_t m_lo = (int64_t) phase + j0 * decim - (ntaps - 1);
        __syncthreads();
        for (int i = tid; i < wsamp; i += kFiltThreads) {
            const int64_t m = m_lo + i;
            uint16_t v = 0;
            if (m >= 0) { if (m < (int64_t) nsamp) v = *reinterpret_cast<const uint16_t *>(src + (uint64_t) m * 2); }
            else if (head && m >= -(int64_t) (ntaps - 1)) v = *reinterpret_cast<const uint16_t *>(head + (uint64_t) ((int64_t) (ntaps - 1) + m) * 2);
            reinterpret_cast<uint16_t *>(win)[i] = v;
        }
        __syncthreads();
        for (int tile = wave; tile * kFiltTileOutputs < n; tile += kFiltThreads / 64) {
            const uint8_t *b_ptr = win + 2 * decim * (kFiltTileOutputs * tile + kFiltColOutputs * col) + 16 * q;
            const uint8_t *a_ptr = filt_lds + lane * 16;
            i32x4 d0 = {0, 0, 0, 0}, d1 = {0, 0, 0, 0};
            for (int t = 0; t < steps; ++t) {
                const i32x4 b = *reinterpret_cast<const i32x4 *>(b_ptr + t * kFiltK);
                const i32x4 a0 = *reinterpret_cast<const i32x4 *>(a_ptr + t * (kFiltK * 16));
                const i32x4 a1 = *reinterpret_cast<const i32x4 *>(a_ptr + (steps + t) * (kFiltK * 16));
                d0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, d0, 0, 0, 0);
                d1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, d1, 0, 0, 0);
            }
            const int o = kFiltTileOutputs * tile + kFiltColOutputs * col + 2 * q;                   // this lane's first output of the run
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (o + s >= n) break;
                const int vi = finish<OUT>(d0[2 * s] + 256 * d1[2 * s], shift, clipped);
                const int vq = finish<OUT>(d0[2 * s + 1] + 256 * d1[2 * s + 1], shift, clipped);
                store_sample<OUT>(dst, (uint64_t) (j0 + o + s), vi, vq);
            }
        }
    }
    count_clipped<kFiltThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_filter.cpp looks up.  nullptr: no such kernel.
FilterGenericFn filter_generic_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? filter_generic<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? filter_generic<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? filter_generic<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? filter_generic<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}

FilterMfmaFn filter_mfma_kernel(int out_fmt)
{
    return out_fmt == GPSIQ_SC08 ? filter_mfma<GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? filter_mfma<GPSIQ_SC16> : nullptr;
}
}  // namespace gpsiq
