// gpsiq_stap_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_stap_cov and gpsiq_stap_combine (include/gpsiq_rows.h,
// "Space-time array"): the exact integer covariance of the K = E T rows z_(e,t)(n) = x_e(n - t) of up to eight streams of interleaved
// I,Q samples, and their weighted sum.
//   stap_cov_generic<FMT>    both formats: a workgroup stages a chunk of every element and the T - 1 samples before it in LDS, the
//                            lanes share the K^2 entries of R out; int32 partials of one chunk (int8) or int64 throughout (int16)
//   stap_cov_mfma<G>         int8 input: the 2 K real rows in G groups of 16, the tiles (g, h), g >= h, of their Gram matrix by
//                            v_mfma_i32_16x16x64_i8 with group g as operand A and group h as operand B (gpsiq_stap_geometry.h has
//                            the tiles, the orientation and the flush bound); a lane's 16 samples of row (e, t) start t samples
//                            before its k-step's, and for odd t come out of nine dwords by a 16-bit funnel shift
//   stap_combine<IN, OUT>    a lane owns a slot, 16 aligned bytes of dst: it reads the slot's samples and the T - 1 before them of
//                            every element, sums them against the weights in int32, rounds, clamps, counts
// Pointers and weights arrive by value as kernel arguments and are wave-uniform.  Every offset into a stream is 64 bits wide.
// Sample n of a source is read only for 0 <= n < nsamp, sample m of a head only for 0 <= m < T - 1, dst is written for
// 0 <= n < nsamp and nowhere else.  No workgroup waits for another: the covariance kernels meet in 64-bit atomic adds into a scratch
// the host has zeroed, and integer addition makes the order of their arrival irrelevant.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_stap_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::load_pair;
using stream::sample_at;
using stream::store_sample;
using stream::count_clipped;

typedef uint32_t stap_u32x4 __attribute__((ext_vector_type(4)));

// entry e of eight pointers: a chain of selects over the argument registers, so that a lane-dependent e needs no table in memory
__device__ __forceinline__ const uint8_t *pointer_of(const uint8_t *const (&p)[kStapMaxElem], int e)
{
    const uint8_t *r = p[0];
#pragma unroll
    for (int k = 1; k < kStapMaxElem; ++k) r = e == k ? p[k] : r;
    return r;
}

// Arguments: the streams and heads, elements, taps, the samples, the runs of the span (gpsiq_stap_plan.h), the scratch as [K][K][2]
// int64 (zeroed by the host).  Workgroup g takes runs g, g + gridDim.x, ... of kStapGenRun samples.  Work item v = tid + 256 j is
// entry v % K^2 at phase v / K^2 of stap_gen_phases(K): below 256 entries a lane has one item and the phases share a chunk's samples,
// from 256 entries on there is one phase and a lane has up to four entries.
template <int FMT>
__global__ __launch_bounds__(kStapThreads) void stap_cov_generic(const StapSources src, int nelem, int ntaps, int nsamp, uint64_t runs,
                                                                 unsigned long long *__restrict__ scratch)
{
    __shared__ uint32_t x[(kStapChunk + kStapMaxTaps - 1) * kStapMaxElem];     // x[i * nelem + e], i = n - c0 + (ntaps - 1)
    __shared__ long long red[kStapThreads][2];
    const int tid = threadIdx.x;
    const int rows = nelem * ntaps, entries = rows * rows, hist = ntaps - 1, phases = stap_gen_phases(rows);
    bool own[kStapGenOwned];
    int at_a[kStapGenOwned], at_b[kStapGenOwned], sub[kStapGenOwned];
    long long re[kStapGenOwned], im[kStapGenOwned];
#pragma unroll
    for (int j = 0; j < kStapGenOwned; ++j) {
        const int v = tid + kStapThreads * j, p = v % entries, k = p / rows, l = p % rows;
        own[j] = v < entries * phases;
        sub[j] = v / entries;
        at_a[j] = (hist - k % ntaps) * nelem + k / ntaps;              // row k at the chunk's sample 0
        at_b[j] = (hist - l % ntaps) * nelem + l / ntaps;
        re[j] = 0;
        im[j] = 0;
    }
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t r0 = (int64_t) r * kStapGenRun;
        const int64_t r1 = r0 + kStapGenRun < (int64_t) nsamp ? r0 + kStapGenRun : (int64_t) nsamp;
        for (int64_t c0 = r0; c0 < r1; c0 += kStapChunk) {
            const int len = r1 - c0 < (int64_t) kStapChunk ? (int) (r1 - c0) : kStapChunk;
            __syncthreads();                                           // the chunk before has been read
            for (int i = tid; i < len + hist; i += kStapThreads)
                for (int e = 0; e < nelem; ++e) x[i * nelem + e] = sample_at<FMT>(src.p[e], src.head[e], c0 - hist + i, nsamp, ntaps);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kStapGenOwned; ++j) {
                if (!own[j]) continue;
                if (FMT == GPSIQ_SC08) {
                    int pr = 0, pi = 0;                                // at most kStapChunk terms of at most 2^15 each
                    for (int n = sub[j]; n < len; n += phases) {
                        const uint32_t va = x[n * nelem + at_a[j]], vb = x[n * nelem + at_b[j]];
                        const int ia = (int) (int16_t) (va & 0xffffu), qa = (int32_t) va >> 16, ib = (int) (int16_t) (vb & 0xffffu), qb = (int32_t) vb >> 16;
                        pr += ia * ib + qa * qb;
                        pi += qa * ib - ia * qb;
                    }
                    re[j] += pr;
                    im[j] += pi;
                } else {
                    for (int n = sub[j]; n < len; n += phases) {
                        const uint32_t va = x[n * nelem + at_a[j]], vb = x[n * nelem + at_b[j]];
                        const long long ia = (int16_t) (va & 0xffffu), qa = (int32_t) va >> 16, ib = (int16_t) (vb & 0xffffu), qb = (int32_t) vb >> 16;
                        re[j] += ia * ib + qa * qb;
                        im[j] += qa * ib - ia * qb;
                    }
                }
            }
        }
    }
    if (phases == 1) {                                                 // (the same for every lane) an entry has one owner
#pragma unroll
        for (int j = 0; j < kStapGenOwned; ++j) {
            if (!own[j]) continue;
            unsigned long long *out = scratch + 2 * (tid + kStapThreads * j);
            if (re[j]) atomicAdd(out, (unsigned long long) re[j]);
            if (im[j]) atomicAdd(out + 1, (unsigned long long) im[j]);
        }
        return;
    }
    red[tid][0] = re[0];                                               // (a lane that owns nothing holds zeros)
    red[tid][1] = im[0];
    __syncthreads();
    if (tid < entries) {
        long long sr = 0, si = 0;
        for (int k = 0; k < phases; ++k) { sr += red[tid + k * entries][0]; si += red[tid + k * entries][1]; }
        unsigned long long *out = scratch + 2 * tid;
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

// The 16 bytes a lane feeds row (e, t) with: component c of z(n0) .. z(n0 + 15), z(n) = x(n - t) for n < nsamp and zero from nsamp
// on -- the row ends where the span does, t samples before the stream -- with x(m) the contract's: the span, the head before it,
// zeros before that and where there is no head.  A window whose rows lie inside the span and whose samples m0 = n0 - t .. m0 + 15 do
// too is 32 bytes at a 2-byte aligned address.  m0 even: 4-byte aligned, two 16-byte loads where it is aligned to that, else eight
// dwords.  m0 odd: the nine dwords from sample m0 - 1 on, shifted down by 16 bits; their last 16 bits are sample m0 + 16, which is
// inside the span because row time n0 + 16 is asked to be.  Any other window goes sample by sample.
__device__ __forceinline__ i32x4 stap_row_bytes(const uint8_t *base, const uint8_t *head, int c, int64_t n0, int t, int ntaps, int nsamp)
{
    i32x4 v = {0, 0, 0, 0};
    if (n0 >= (int64_t) nsamp) return v;
    const int64_t m0 = n0 - t;
    const int odd = (int) (m0 & 1);
    if (m0 >= 0 && n0 + kStapLaneSamples + odd <= (int64_t) nsamp) {
        const uint8_t *p = base + (uint64_t) (m0 - odd) * 2;           // 4-byte aligned
        uint32_t w[8];
        if (odd) {
            uint32_t d[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) d[j] = reinterpret_cast<const uint32_t *>(p)[j];
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = (d[j] >> 16) | (d[j + 1] << 16);
        } else if (!((uintptr_t) p & 15)) {
            const stap_u32x4 lo = reinterpret_cast<const stap_u32x4 *>(p)[0], hi = reinterpret_cast<const stap_u32x4 *>(p)[1];
            w[0] = lo[0]; w[1] = lo[1]; w[2] = lo[2]; w[3] = lo[3]; w[4] = hi[0]; w[5] = hi[1]; w[6] = hi[2]; w[7] = hi[3];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = reinterpret_cast<const uint32_t *>(p)[j];
        }
        return pick_component(w, c);
    }
    const int left = n0 + kStapLaneSamples <= (int64_t) nsamp ? kStapLaneSamples : (int) ((int64_t) nsamp - n0);     // rows of the window inside the span
#pragma unroll
    for (int i = 0; i < kStapLaneSamples; ++i) {
        if (i >= left) break;
        const uint32_t pair = sample_at<GPSIQ_SC08>(base, head, m0 + i, nsamp, ntaps);
        v[i >> 2] |= (int) (((pair >> (16 * c)) & 0xffu) << (8 * (i & 3)));
    }
    return v;
}

// Arguments: the streams and heads (int8), elements, taps, the samples, the k-steps of the span and of a workgroup's run
// (gpsiq_stap_plan.h), the scratch as the real Gram matrix [64][64] int64 (zeroed by the host).  Workgroup b takes k-steps
// [b run, b run + run), wave w of it every fourth from b run + w.
// Lanes (gpsiq_acquire_kernels.hip measured the map): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds column
// l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2).  For group g lane l holds component (l & 1) of
// row k = 8 g + ((l & 15) >> 1), element k / ntaps at tap t = k % ntaps, at samples 64 s + 16 (l >> 4) + j - t of k-step s (zero where 64 s + 16 (l >> 4) + j >= nsamp); tile
// (g, h) takes group g's registers as A and group h's as B, so its D(i, j) belongs to real rows (16 g + i, 16 h + j).
template <int G>
__global__ __launch_bounds__(kStapThreads) void stap_cov_mfma(const StapSources src, int nelem, int ntaps, int nsamp, uint64_t steps, uint64_t run,
                                                              unsigned long long *__restrict__ gram)
{
    constexpr int T = stap_tiles(G);
    __shared__ long long red[kStapWaves][kStapTileWords];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, row = lane & 15, q = lane >> 4;
    const int rows = nelem * ntaps, c = row & 1;
    const uint8_t *base[G], *head[G];
    int tap[G];
    bool live[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int k = 8 * g + (row >> 1);
        live[g] = k < rows;
        const int e = live[g] ? k / ntaps : 0;
        tap[g] = k % ntaps;
        base[g] = pointer_of(src.p, e);
        head[g] = pointer_of(src.head, e);
    }
    const uint64_t s_begin = (uint64_t) blockIdx.x * run, s_end = s_begin + run < steps ? s_begin + run : steps;
    long long sum[T][4];
    i32x4 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        acc[t] = i32x4{0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[t][r] = 0;
    }
    int pending = 0;
    for (uint64_t s = s_begin + (uint64_t) wave; s < s_end; s += kStapWaves) {
        const int64_t n0 = (int64_t) (s * kStapK) + kStapLaneSamples * q;
        i32x4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            v[g] = i32x4{0, 0, 0, 0};
            if (live[g]) v[g] = stap_row_bytes(base[g], head[g], c, n0, tap[g], ntaps, nsamp);
        }
        {
            int t = 0;
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int h = 0; h <= g; ++h, ++t) acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(v[g], v[h], acc[t], 0, 0, 0);
        }
        if (++pending == kStapFlushSteps) {                            // (the same for every lane of the wave)
#pragma unroll
            for (int t = 0; t < T; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sum[t][r] += acc[t][r];
                acc[t] = i32x4{0, 0, 0, 0};
            }
            pending = 0;
        }
    }
    int t = 0;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int h = 0; h <= g; ++h, ++t) {
            __syncthreads();                                           // the tile before has been read
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][(4 * q + r) * kStapTile + row] = sum[t][r] + acc[t][r];     // D(4 q + r, col = lane & 15)
            __syncthreads();
            long long total = 0;
#pragma unroll
            for (int w = 0; w < kStapWaves; ++w) total += red[w][tid];
            if (total) atomicAdd(gram + (kStapTile * g + (tid >> 4)) * kStapRealRows + kStapTile * h + (tid & 15), (unsigned long long) total);
        }
}

// Arguments: the streams and heads, the weights (row e T + t: re in the low half of a word, im in the high half), elements, taps, the
// samples, shift, the destination, the samples of the first slot that lie before sample 0, the slots of the launch
// (gpsiq_stap_plan.h), the counter (zeroed by the host).  Slot u holds samples u S - lead .. u S - lead + S - 1, those of them in
// [0, nsamp); its first byte is 16-byte aligned.  Thread t of the launch takes slots t, t + gridDim.x * kStapThreads, ...  A lane
// keeps a window of an element, the S + 7 samples that end with the slot's last, in registers: place j is sample n0 - 7 + j, and the
// places below 8 - ntaps are not read.  |acc| <= 65535 * 32768 < 2^31 by the host's bound on the weights.
template <int IN, int OUT>
__global__ __launch_bounds__(kStapThreads) void stap_combine(const StapSources src, const StapWeights wt, int nelem, int ntaps, int nsamp, int shift,
                                                             uint8_t *__restrict__ dst, int lead, uint64_t slots, unsigned long long *__restrict__ count)
{
    constexpr int S = stap_slot_samples(OUT), H = kStapMaxTaps - 1, W = S + H;
    unsigned clipped = 0;
    const int first = H - (ntaps - 1);
    const uint64_t stride = (uint64_t) gridDim.x * kStapThreads;
    for (uint64_t u = (uint64_t) blockIdx.x * kStapThreads + threadIdx.x; u < slots; u += stride) {
        const int64_t n0 = (int64_t) u * S - lead;
        const int lo = n0 < 0 ? (int) -n0 : 0;
        const int64_t left = (int64_t) nsamp - n0;
        const int hi = left < S ? (int) left : S;
        const bool whole = lo == 0 && hi == S;
        const bool inside = whole && n0 >= (int64_t) (ntaps - 1);      // every sample the slot reads is in the span
        int ai[S], aq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) { ai[i] = 0; aq[i] = 0; }
        for (int e = 0; e < nelem; ++e) {
            const uint8_t *p = src.p[e], *hd = src.head[e];
            int xi[W], xq[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                uint32_t v = 0u;
                if (j >= first) v = inside ? load_pair<IN>(p, n0 - H + j) : sample_at<IN>(p, hd, n0 - H + j, nsamp, ntaps);
                xi[j] = (int) (int16_t) (v & 0xffffu);
                xq[j] = (int32_t) v >> 16;
            }
#pragma unroll
            for (int t = 0; t < kStapMaxTaps; ++t) {
                if (t >= ntaps) break;
                const uint32_t w = wt.w[e * ntaps + t];
                const int re = (int) (int16_t) (w & 0xffffu), im = (int32_t) w >> 16;
#pragma unroll
                for (int i = 0; i < S; ++i) {
                    ai[i] += re * xi[H + i - t] - im * xq[H + i - t];
                    aq[i] += re * xq[H + i - t] + im * xi[H + i - t];
                }
            }
        }
        int oi[S], oq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            oi[i] = 0; oq[i] = 0;
            if (i >= lo && i < hi) {                                   // (a place outside the span still sums its neighbours: not an output)
                oi[i] = stream::finish<OUT>(ai[i], shift, clipped);
                oq[i] = stream::finish<OUT>(aq[i], shift, clipped);
            }
        }
        if (whole) {
            stap_u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (OUT == GPSIQ_SC16) v[j] = ((uint32_t) oi[j] & 0xffffu) | ((uint32_t) oq[j] << 16);
                else v[j] = ((uint32_t) oi[2 * j] & 0xffu) | (((uint32_t) oq[2 * j] & 0xffu) << 8) | (((uint32_t) oi[2 * j + 1] & 0xffu) << 16) |
                            ((uint32_t) oq[2 * j + 1] << 24);
            }
            *reinterpret_cast<stap_u32x4 *>(dst + (uint64_t) n0 * (2 * OUT)) = v;
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i)
                if (i >= lo && i < hi) store_sample<OUT>(dst, (uint64_t) (n0 + i), oi[i], oq[i]);
        }
    }
    count_clipped<kStapThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_stap.cpp looks up.  nullptr: no such kernel.
StapCovFn stap_cov_generic_kernel(int fmt)
{
    return fmt == GPSIQ_SC08 ? stap_cov_generic<GPSIQ_SC08> : fmt == GPSIQ_SC16 ? stap_cov_generic<GPSIQ_SC16> : nullptr;
}

StapCovMfmaFn stap_cov_mfma_kernel(int fmt, int groups)
{
    if (fmt != GPSIQ_SC08) return nullptr;
    return groups == 1 ? stap_cov_mfma<1> : groups == 2 ? stap_cov_mfma<2> : groups == 3 ? stap_cov_mfma<3> : groups == 4 ? stap_cov_mfma<4> : nullptr;
}

StapCombineFn stap_combine_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? stap_combine<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? stap_combine<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? stap_combine<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? stap_combine<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}
}  // namespace gpsiq
