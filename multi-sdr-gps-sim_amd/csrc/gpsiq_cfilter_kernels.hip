// gpsiq_cfilter_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_cfilter (include/gpsiq_rows.h, "Complex filter and notch"):
// gpsiq_filter's contract with complex taps h = re + j im over x = I + j Q,
//   accI = sum re[k] I(m_j - k) - im[k] Q(m_j - k),   accQ = sum re[k] Q(m_j - k) + im[k] I(m_j - k).
//   cfilter_generic<IN, OUT>   every format pair, every legal shape: filter_generic's staging, the taps as one dword each (re below, im
//                              above), four int32 MACs per tap and output
//   cfilter_mfma16<OUT>        int16 input: v_mfma_i32_16x16x64_i8 over two byte planes of the stream against the two digit planes of
//                              the taps (gpsiq_cfilter_geometry.h)
// An int8 input on the matrix path is filter_mfma<OUT> of gpsiq_filter_kernels.hip itself, launched with the complex planes.
// sum (|re[k]| + |im[k]|) <= 65535 (checked on the host) and |x| <= 32768 give |acc| <= 2^31 - 32768: one accumulator width, no
// saturation inside the sum.  sample_at(), finish(), store_sample() and count_clipped() are gpsiq_stream.h's, as gpsiq_filter_kernels.hip's
// are.
// Every offset into src / dst is 64 bits wide.  Sample m of the span is read only for 0 <= m < nsamp, sample m < 0 from head (or as
// zero); outputs j < nout are written and nothing else.  No workgroup waits for another; a workgroup strides over the runs.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_cfilter_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::sample_at;
using stream::finish;
using stream::store_sample;
using stream::count_clipped;

// Arguments: span and its samples, head (may be null), device taps as dwords (re low, im high), ntaps, shift, decim, phase,
// destination, outputs of the span, outputs of a run, runs of the launch (gpsiq_cfilter_plan.h), the counter (zeroed by the host).
// Dynamic LDS: [(run - 1) * decim + ntaps] window dwords, [ntaps] taps.
// The four products of a tap are each at most 32768 * 32768 = 2^30 in magnitude and every partial sum is bounded by the tap sum times
// 32768 < 2^31: int32 throughout.
template <int IN, int OUT>
__global__ __launch_bounds__(kFiltThreads) void cfilter_generic(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                                 const uint32_t *__restrict__ taps, int ntaps, int shift, int decim, int phase,
                                                                 uint8_t *__restrict__ dst, int nout, int run, uint64_t runs,
                                                                 unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t cfilt_lds[];
    uint32_t *win = reinterpret_cast<uint32_t *>(cfilt_lds);
    uint32_t *tap = win + ((run - 1) * decim + ntaps);
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
                const uint32_t v = x[-k], t = tap[k];
                const int xi = (int) (int16_t) (v & 0xffffu), xq = (int32_t) v >> 16;
                const int re = (int) (int16_t) (t & 0xffffu), im = (int32_t) t >> 16;
                ai += re * xi - im * xq;
                aq += re * xq + im * xi;
            }
            store_sample<OUT>(dst, (uint64_t) (j0 + o), finish<OUT>(ai, shift, clipped), finish<OUT>(aq, shift, clipped));
        }
    }
    count_clipped<kFiltThreads>(clipped, count);
}

// Arguments as cfilter_generic's, with the digit planes in the taps' place, the k-steps of a tile behind the run, and the two row
// constants 128 sum (re - im), 128 sum (re + im) (gpsiq_cfilter_geometry.h).
// Dynamic LDS: [2][steps][64][16] plane bytes in fragment order, then the lo' window of the run, then its hi window, each
// filter_mfma_window_bytes() long and 16-byte aligned (64 steps bytes plus a multiple of 32).
// Lanes (gpsiq_acquire_kernels.hip measured the map, filter_mfma restates it): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j,
// B lane l feeds column l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2): lane (col, q) ends with I
// and Q of outputs 2 q and 2 q + 1 of column col.
// Four MFMAs per k-step: d0 x lo', d0 x hi, d1 x lo', d1 x hi; the two middle ones share an accumulator.  With 2 ntaps entries a row,
// sum |d0| <= 128 * 1024 and sum |d1| < 768, stream bytes of magnitude <= 128: |P00|, |P01| <= 2^24, |P10|, |P11| < 2^17, so every
// accumulator, and P01 + P10, is inside int32.  The recombination P00 + 256 (P01 + P10) + 65536 P11 + const is NOT term by term
// (|65536 P11| can pass 2^32), but its value is acc, |acc| < 2^31: it is added in uint32, modulo 2^32, and read back as int32 -- exact.
// A window position the contract calls zero (before the head, no head, past the span, the padding of the last tile) is staged as
// (lo' = -128, hi = 0): the constant is added to every row alike.
template <int OUT>
__global__ __launch_bounds__(kFiltThreads) void cfilter_mfma16(const uint8_t *__restrict__ src, int nsamp, const uint8_t *__restrict__ head,
                                                                const uint8_t *__restrict__ planes, int ntaps, int shift, int decim, int phase,
                                                                uint8_t *__restrict__ dst, int nout, int run, uint64_t runs, int steps,
                                                                int const_i, int const_q, unsigned long long *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t cfilt_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int plane_bytes = filter_mfma_plane_bytes(steps);
    const int wbytes = filter_mfma_window_bytes(run, decim, steps);
    uint8_t *win_lo = cfilt_lds + plane_bytes, *win_hi = win_lo + wbytes;
    const int wsamp = wbytes / 2;                                                                    // samples staged per run
    for (int i = tid; i < plane_bytes / 16; i += kFiltThreads)
        reinterpret_cast<i32x4 *>(cfilt_lds)[i] = reinterpret_cast<const i32x4 *>(planes)[i];
    const int col = lane & 15, q = lane >> 4;
    unsigned clipped = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t j0 = (int64_t) r * run;
        const int n = (int64_t) nout - j0 < (int64_t) run ? (int) ((int64_t) nout - j0) : run;
        const int64_t m_lo = (int64_t) phase + j0 * decim - (ntaps - 1);
        __syncthreads();
        for (int i = tid; i < wsamp; i += kFiltThreads) {
            const uint32_t v = sample_at<GPSIQ_SC16>(src, head, m_lo + i, nsamp, ntaps);             // 0: the contract's zero
            reinterpret_cast<uint16_t *>(win_lo)[i] = (uint16_t) (((v & 0xffu) | ((v >> 8) & 0xff00u)) ^ 0x8080u);      // (x & 255) - 128 as a byte
            reinterpret_cast<uint16_t *>(win_hi)[i] = (uint16_t) (((v >> 8) & 0xffu) | ((v >> 16) & 0xff00u));         // x >> 8
        }
        __syncthreads();
        for (int tile = wave; tile * kFiltTileOutputs < n; tile += kFiltThreads / 64) {
            const int b_off = 2 * decim * (kFiltTileOutputs * tile + kFiltColOutputs * col) + 16 * q;
            const uint8_t *lo_ptr = win_lo + b_off, *hi_ptr = win_hi + b_off;
            const uint8_t *a_ptr = cfilt_lds + lane * 16;
            i32x4 p00 = {0, 0, 0, 0}, pmid = {0, 0, 0, 0}, p11 = {0, 0, 0, 0};
            for (int t = 0; t < steps; ++t) {
                const i32x4 lo = *reinterpret_cast<const i32x4 *>(lo_ptr + t * kFiltK);
                const i32x4 hi = *reinterpret_cast<const i32x4 *>(hi_ptr + t * kFiltK);
                const i32x4 a0 = *reinterpret_cast<const i32x4 *>(a_ptr + t * (kFiltK * 16));
                const i32x4 a1 = *reinterpret_cast<const i32x4 *>(a_ptr + (steps + t) * (kFiltK * 16));
                p00 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, lo, p00, 0, 0, 0);
                pmid = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, hi, pmid, 0, 0, 0);
                pmid = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, lo, pmid, 0, 0, 0);
                p11 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, hi, p11, 0, 0, 0);
            }
            const int o = kFiltTileOutputs * tile + kFiltColOutputs * col + 2 * q;                   // this lane's first output of the run
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (o + s >= n) break;
                const uint32_t ui = (uint32_t) p00[2 * s] + ((uint32_t) pmid[2 * s] << 8) + ((uint32_t) p11[2 * s] << 16) + (uint32_t) const_i;
                const uint32_t uq = (uint32_t) p00[2 * s + 1] + ((uint32_t) pmid[2 * s + 1] << 8) + ((uint32_t) p11[2 * s + 1] << 16) + (uint32_t) const_q;
                store_sample<OUT>(dst, (uint64_t) (j0 + o + s), finish<OUT>((int) ui, shift, clipped), finish<OUT>((int) uq, shift, clipped));
            }
        }
    }
    count_clipped<kFiltThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_cfilter.cpp looks up.  nullptr: no such kernel.
CfilterGenericFn cfilter_generic_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? cfilter_generic<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? cfilter_generic<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? cfilter_generic<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? cfilter_generic<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}

CfilterMfma16Fn cfilter_mfma16_kernel(int out_fmt)
{
    return out_fmt == GPSIQ_SC08 ? cfilter_mfma16<GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? cfilter_mfma16<GPSIQ_SC16> : nullptr;
}
}  // namespace gpsiq
