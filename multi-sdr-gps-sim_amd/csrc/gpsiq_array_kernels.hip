// gpsiq_array_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_array_cov and gpsiq_array_combine (include/gpsiq_rows.h, "Array"):
// the exact integer covariance of up to eight streams of interleaved I,Q samples, and their weighted sum.
//   array_cov_generic<FMT>   both formats: a workgroup stages a chunk of every element in LDS, a lane owns one entry R[a][b] and
//                            every k-th sample of the chunk; int32 partials of one chunk (int8) or int64 throughout (int16)
//   array_cov_mfma           int8 input: v_mfma_i32_16x16x64_i8 with the same 64 samples as both operands, the 2 E rows I_0, Q_0, ...
//                            de-interleaved from the loaded dwords (gpsiq_array_geometry.h has the tile and the flush bound)
//   array_combine<IN, OUT>   a lane owns a slot, 16 aligned bytes of dst: it reads the slot's samples of every element in the widest
//                            loads the address allows, sums them against the weights in int32, rounds, clamps, counts
// Pointers and weights arrive by value as kernel arguments and are wave-uniform.  Every offset into a stream is 64 bits wide.
// Sample n of a source is read only for 0 <= n < nsamp, dst is written for 0 <= n < nsamp and nowhere else.  No workgroup waits
// for another: the covariance kernels meet in 64-bit atomic adds into a scratch the host has zeroed, and integer addition makes
// the order of their arrival irrelevant.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_array_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::load_pair;
using stream::store_sample;
using stream::count_clipped;

typedef uint32_t arr_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t arr_u32x2 __attribute__((ext_vector_type(2)));

// element e's stream: a chain of selects over the argument registers, so that a lane-dependent e needs no table in memory
__device__ __forceinline__ const uint8_t *stream_of(const ArraySources &src, int e)
{
    const uint8_t *p = src.p[0];
#pragma unroll
    for (int k = 1; k < kArrMaxElem; ++k) p = e == k ? src.p[k] : p;
    return p;
}

// Arguments: the streams, their number, the samples, the runs of the span (gpsiq_array_plan.h), the scratch as [8][8][2] int64
// (zeroed by the host).  Workgroup g takes runs g, g + gridDim.x, ... of kArrGenRun samples.
template <int FMT>
__global__ __launch_bounds__(kArrThreads) void array_cov_generic(const ArraySources src, int nelem, int nsamp, uint64_t runs,
                                                                 unsigned long long *__restrict__ scratch)
{
    __shared__ uint32_t x[kArrChunk * kArrMaxElem];                    // x[n * pw + e]
    __shared__ long long red[kArrThreads][2];
    const int tid = threadIdx.x;
    const int pw = array_pair_width(nelem), pairs = pw * pw, phases = kArrThreads / pairs;
    const int p = tid % pairs, a = p / pw, b = p % pw, sub = tid / pairs;
    long long re = 0, im = 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t r0 = (int64_t) r * kArrGenRun;
        const int64_t r1 = r0 + kArrGenRun < (int64_t) nsamp ? r0 + kArrGenRun : (int64_t) nsamp;
        for (int64_t c0 = r0; c0 < r1; c0 += kArrChunk) {
            const int len = r1 - c0 < (int64_t) kArrChunk ? (int) (r1 - c0) : kArrChunk;
            __syncthreads();                                           // the chunk before has been read
            if (tid < len)
                for (int e = 0; e < pw; ++e) x[tid * pw + e] = e < nelem ? load_pair<FMT>(src.p[e], c0 + tid) : 0u;
            __syncthreads();
            if (FMT == GPSIQ_SC08) {
                int pr = 0, pi = 0;                                    // at most kArrChunk terms of at most 2^15 each
                for (int n = sub; n < len; n += phases) {
                    const uint32_t va = x[n * pw + a], vb = x[n * pw + b];
                    const int ia = (int) (int16_t) (va & 0xffffu), qa = (int32_t) va >> 16, ib = (int) (int16_t) (vb & 0xffffu), qb = (int32_t) vb >> 16;
                    pr += ia * ib + qa * qb;
                    pi += qa * ib - ia * qb;
                }
                re += pr;
                im += pi;
            } else {
                for (int n = sub; n < len; n += phases) {
                    const uint32_t va = x[n * pw + a], vb = x[n * pw + b];
                    const long long ia = (int16_t) (va & 0xffffu), qa = (int32_t) va >> 16, ib = (int16_t) (vb & 0xffffu), qb = (int32_t) vb >> 16;
                    re += ia * ib + qa * qb;
                    im += qa * ib - ia * qb;
                }
            }
        }
    }
    red[tid][0] = re;
    red[tid][1] = im;
    __syncthreads();
    if (tid < pairs && a < nelem && b < nelem) {
        long long sr = 0, si = 0;
        for (int k = 0; k < phases; ++k) { sr += red[tid + k * pairs][0]; si += red[tid + k * pairs][1]; }
        unsigned long long *out = scratch + 2 * kArrMaxElem * a + 2 * b;
        if (sr) atomicAdd(out, (unsigned long long) sr);
        if (si) atomicAdd(out + 1, (unsigned long long) si);
    }
}

// byte c of every pair of bytes of eight dwords, in order: 16 samples' component c (shifts and masks: a byte permute)
__device__ __forceinline__ i32x4 pick_component(const uint32_t *w, int c)
{
    i32x4 v;
    const int sh = 8 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t w0 = w[2 * j] >> sh, w1 = w[2 * j + 1] >> sh;
        v[j] = (int) ((w0 & 0xffu) | ((w0 >> 8) & 0xff00u) | ((w1 & 0xffu) << 16) | ((w1 << 8) & 0xff000000u));
    }
    return v;
}

// The 16 bytes a lane feeds its row with: component c of samples n0 .. n0 + 15 of the stream at base, all of them inside the span
// and the address 16-byte aligned: two 16-byte loads
__device__ __forceinline__ i32x4 gram_row_aligned(const uint8_t *base, int c, int64_t n0)
{
    const arr_u32x4 *p = reinterpret_cast<const arr_u32x4 *>(base + (uint64_t) n0 * 2);
    const arr_u32x4 lo = p[0], hi = p[1];
    const uint32_t w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return pick_component(w, c);
}

// The same for any run: zeros from nsamp on.  A whole run is 32 bytes at a 4-byte aligned address (n0 is a multiple of 16): two
// 16-byte loads where it is aligned to that, else eight dwords.  A run the span ends in goes byte by byte.
__device__ __forceinline__ i32x4 gram_row_bytes(const uint8_t *base, int c, int64_t n0, int nsamp)
{
    i32x4 v = {0, 0, 0, 0};
    if (n0 >= (int64_t) nsamp) return v;
    const uint8_t *p = base + (uint64_t) n0 * 2;
    if (n0 + kArrLaneSamples <= (int64_t) nsamp) {
        if (!((uintptr_t) p & 15)) return gram_row_aligned(base, c, n0);
        uint32_t w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = reinterpret_cast<const uint32_t *>(p)[j];
        return pick_component(w, c);
    }
    const int left = (int) ((int64_t) nsamp - n0);                     // 1 .. 15
#pragma unroll
    for (int i = 0; i < kArrLaneSamples; ++i)
        if (i < left) v[i >> 2] |= (int) ((uint32_t) p[2 * i + c] << (8 * (i & 3)));
    return v;
}

// Arguments: the streams (int8), their number, the samples, the k-steps of the span and of a workgroup's run (gpsiq_array_plan.h),
// the scratch as the Gram tile [16][16] int64 (zeroed by the host).  Workgroup g takes k-steps [g run, g run + run), wave w of it
// every fourth from g run + w.
// Lanes (gpsiq_acquire_kernels.hip measured the map): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds
// column l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2).  Here A and B are the same four
// registers: lane l holds component (l & 1) of element (l & 15) >> 1 at samples 64 s + 16 (l >> 4) + j of k-step s.
__global__ __launch_bounds__(kArrThreads) void array_cov_mfma(const ArraySources src, int nelem, int nsamp, uint64_t steps, uint64_t run,
                                                              unsigned long long *__restrict__ gram)
{
    __shared__ long long red[kArrWaves][kArrGramWords];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane & 15, q = lane >> 4;
    const int e = row >> 1, c = row & 1;
    const bool live = e < nelem;
    const uint8_t *base = stream_of(src, e);
    const uint64_t s_begin = (uint64_t) blockIdx.x * run, s_end = s_begin + run < steps ? s_begin + run : steps;
    long long sum[4] = {0, 0, 0, 0};
    i32x4 acc = {0, 0, 0, 0};
    int pending = 0;
    for (uint64_t s = s_begin + (uint64_t) wave; s < s_end; s += kArrWaves) {
        i32x4 v = {0, 0, 0, 0};
        if (live) v = gram_row_bytes(base, c, (int64_t) (s * kArrK) + kArrLaneSamples * q, nsamp);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(v, v, acc, 0, 0, 0);
        if (++pending == kArrFlushSteps) {                             // (the same for every lane of the wave)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[r] += acc[r];
            acc = i32x4{0, 0, 0, 0};
            pending = 0;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sum[r] += acc[r];
        red[wave][(4 * q + r) * kArrRows + row] = sum[r];              // D(4 q + r, col = lane & 15)
    }
    __syncthreads();
    long long total = 0;
#pragma unroll
    for (int w = 0; w < kArrWaves; ++w) total += red[w][tid];
    if (total) atomicAdd(gram + tid, (unsigned long long) total);
}

// S whole samples of a stream at p into dwords of (I low, Q high, sign-extended): dword loads where p is 4-byte aligned (always
// for int16; for int8 unless the slot starts at an odd sample), as 16- or 8-byte loads where p is aligned to that too
template <int FMT, int S>
__device__ __forceinline__ void load_slot(const uint8_t *p, int *xi, int *xq)
{
    constexpr int W = S * 2 * FMT / 4;                                 // dwords of the run: 2, 4 or 8
    const uintptr_t a = (uintptr_t) p;
    if (FMT == GPSIQ_SC08 && (a & 3)) {
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const uint32_t v = load_pair<FMT>(p, i);
            xi[i] = (int) (int16_t) (v & 0xffffu);
            xq[i] = (int32_t) v >> 16;
        }
        return;
    }
    uint32_t w[W];
    if (W >= 4 && !(a & 15)) {
#pragma unroll
        for (int j = 0; j < W / 4; ++j) {
            const arr_u32x4 v = reinterpret_cast<const arr_u32x4 *>(p)[j];
            w[4 * j] = v[0]; w[4 * j + 1] = v[1]; w[4 * j + 2] = v[2]; w[4 * j + 3] = v[3];
        }
    } else if (W == 2 && !(a & 7)) {
        const arr_u32x2 v = *reinterpret_cast<const arr_u32x2 *>(p);
        w[0] = v[0]; w[1] = v[1];
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) w[j] = reinterpret_cast<const uint32_t *>(p)[j];
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        if (FMT == GPSIQ_SC16) {
            xi[i] = (int) (int16_t) (w[i] & 0xffffu);
            xq[i] = (int32_t) w[i] >> 16;
        } else {
            const uint32_t h = w[i >> 1] >> (16 * (i & 1));
            xi[i] = (int) (int8_t) (h & 0xffu);
            xq[i] = (int) (int8_t) ((h >> 8) & 0xffu);
        }
    }
}

// Arguments: the streams, the weights (re in the low half of a word, im in the high half), their number, the samples, shift, the
// destination, the samples of the first slot that lie before sample 0, the slots of the launch (gpsiq_array_plan.h), the counter
// (zeroed by the host).  Slot u holds samples u S - lead .. u S - lead + S - 1, those of them in [0, nsamp); its first byte is
// 16-byte aligned.  Thread t of the launch takes slots t, t + gridDim.x * kArrThreads, ...: the lanes of a wave write 1 KiB back to
// back.  |acc| <= 65535 * 32768 < 2^31 by the host's bound on the weights.
template <int IN, int OUT>
__global__ __launch_bounds__(kArrThreads) void array_combine(const ArraySources src, const ArrayWeights wt, int nelem, int nsamp, int shift,
                                                             uint8_t *__restrict__ dst, int lead, uint64_t slots, unsigned long long *__restrict__ count)
{
    constexpr int S = array_slot_samples(OUT);
    unsigned clipped = 0;
    const uint64_t stride = (uint64_t) gridDim.x * kArrThreads;
    for (uint64_t u = (uint64_t) blockIdx.x * kArrThreads + threadIdx.x; u < slots; u += stride) {
        const int64_t n0 = (int64_t) u * S - lead;
        const int lo = n0 < 0 ? (int) -n0 : 0;
        const int64_t left = (int64_t) nsamp - n0;
        const int hi = left < S ? (int) left : S;
        const bool whole = lo == 0 && hi == S;
        int ai[S], aq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) { ai[i] = 0; aq[i] = 0; }
        for (int e = 0; e < nelem; ++e) {
            const int re = (int) (int16_t) (wt.w[e] & 0xffffu), im = (int32_t) wt.w[e] >> 16;
            int xi[S], xq[S];
            if (whole) load_slot<IN, S>(src.p[e] + (uint64_t) n0 * (2 * IN), xi, xq);
            else {
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    const uint32_t v = i >= lo && i < hi ? load_pair<IN>(src.p[e], n0 + i) : 0u;
                    xi[i] = (int) (int16_t) (v & 0xffffu);
                    xq[i] = (int32_t) v >> 16;
                }
            }
#pragma unroll
            for (int i = 0; i < S; ++i) {
                ai[i] += re * xi[i] - im * xq[i];
                aq[i] += re * xq[i] + im * xi[i];
            }
        }
        int oi[S], oq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            // (a sample outside the span is a sum of zeros: nothing to clamp, nothing counted)
            oi[i] = stream::finish<OUT>(ai[i], shift, clipped);
            oq[i] = stream::finish<OUT>(aq[i], shift, clipped);
        }
        if (whole) {
            arr_u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (OUT == GPSIQ_SC16) v[j] = ((uint32_t) oi[j] & 0xffffu) | ((uint32_t) oq[j] << 16);
                else v[j] = ((uint32_t) oi[2 * j] & 0xffu) | (((uint32_t) oq[2 * j] & 0xffu) << 8) | (((uint32_t) oi[2 * j + 1] & 0xffu) << 16) |
                            ((uint32_t) oq[2 * j + 1] << 24);
            }
            *reinterpret_cast<arr_u32x4 *>(dst + (uint64_t) n0 * (2 * OUT)) = v;
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i)
                if (i >= lo && i < hi) store_sample<OUT>(dst, (uint64_t) (n0 + i), oi[i], oq[i]);
        }
    }
    count_clipped<kArrThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_array.cpp looks up.  nullptr: no such kernel.
ArrayCovFn array_cov_generic_kernel(int fmt)
{
    return fmt == GPSIQ_SC08 ? array_cov_generic<GPSIQ_SC08> : fmt == GPSIQ_SC16 ? array_cov_generic<GPSIQ_SC16> : nullptr;
}

ArrayCovMfmaFn array_cov_mfma_kernel(int fmt) { return fmt == GPSIQ_SC08 ? array_cov_mfma : nullptr; }

ArrayCombineFn array_combine_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? array_combine<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? array_combine<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? array_combine<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? array_combine<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}
}  // namespace gpsiq
