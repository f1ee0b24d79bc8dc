// gpsiq_agc_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_agc / gpsiq_generate_batch_agc (include/gpsiq_rows.h, "AGC"): a
// device stream (interleaved I,Q, int8 or int16, one contiguous span) through a blanker with an absolute threshold, a gain that is
// constant over a window and a function of the exact power sums of the windows before it, and a counted clamp.  Three launches per span:
//   agc_measure<IN_FMT, MASK>          blank flags (MASK: exceed flags, the last exceeding sample at or before every sample as a prefix
//                                      maximum over the tile and a lead-in of blank_hold samples read again from the span, one mask
//                                      byte per unit), and per window the sum of squares and the count of the unblanked elements:
//                                      per lane, per wave where a wave lies inside one window, per workgroup in LDS, then one 64-bit
//                                      and one 32-bit atomic per workgroup and window.  Integer addition: the order of arrival does not
//                                      matter.  The last tile writes the hold the span leaves
//   agc_gains                          one thread per touched window: up to navg earlier windows from the state's ring and from this
//                                      span's slots, the gain rule (gpsiq_agc_geometry.h); the first workgroup writes the state out
//   agc_apply<IN_FMT, OUT_FMT, MASK>   element-wise: multiply, round, clamp, count, store
// A lane works on UNITS of 8 samples (gpsiq_agc_geometry.h): 16 or 32 source bytes in 16-byte loads, 16 or 32 destination bytes in
// 16-byte stores, one mask byte.  Span and destination are 4-byte aligned and no more, so every wide access is declared with 4-byte
// alignment, as in the packer.  A unit is wide only where ALL of it lies inside the span; the one ragged unit at the span's end goes
// element by element: a byte behind the span is never read, a byte behind 2 * nsamp elements of the destination never written.
// With the blanker off (MASK false) no mask exists: a sample is blanked iff it lies in the hold handed in.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_agc_geometry.h"

namespace gpsiq {
namespace {

struct Quad { uint32_t w[4]; };

// 16 bytes at a 4-byte aligned address
__device__ __forceinline__ Quad load16(const uint8_t *p)
{
    Quad v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 16);
    return v;
}
__device__ __forceinline__ void store16(uint8_t *p, const Quad &v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 16); }

constexpr int kNone = -(1 << 20);              // "no exceeding sample": further back than any hold, relative to any tile

// the 2 * kAgcUnit elements of the unit whose first sample is m0, of which n samples lie inside the span; the others read as zeros
template <int FMT>
__device__ __forceinline__ void load_unit(const uint8_t *__restrict__ src, uint64_t m0, int n, int *x)
{
    if (n == kAgcUnit) {
        if (FMT == GPSIQ_SC08) {
            const Quad q = load16(src + m0 * 2);
#pragma unroll
            for (int e = 0; e < 16; ++e) x[e] = (int) (int8_t) (q.w[e >> 2] >> (8 * (e & 3)));
        } else {
            const Quad a = load16(src + m0 * 4), b = load16(src + m0 * 4 + 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                x[e] = (int) (int16_t) (a.w[e >> 1] >> (16 * (e & 1)));
                x[8 + e] = (int) (int16_t) (b.w[e >> 1] >> (16 * (e & 1)));
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            x[e] = 0;
            if (e < 2 * n) x[e] = FMT == GPSIQ_SC16 ? (int) reinterpret_cast<const int16_t *>(src)[2 * m0 + e] : (int) reinterpret_cast<const int8_t *>(src)[2 * m0 + e];
        }
    }
}

// bit j: sample j of the unit exceeds (zeros never do: the threshold is at least 1)
__device__ __forceinline__ uint32_t exceed_bits(const int *x, int thresh)
{
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kAgcUnit; ++j) {
        const int i = x[2 * j] < 0 ? -x[2 * j] : x[2 * j], q = x[2 * j + 1] < 0 ? -x[2 * j + 1] : x[2 * j + 1];
        bits |= (uint32_t) (i > thresh || q > thresh) << j;
    }
    return bits;
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

// Arguments: gpsiq_agc.h.  One workgroup per tile; lane t of it has unit t of the tile.
template <int FMT, bool MASK>
__global__ __launch_bounds__(kAgcThreads) void agc_measure(const uint8_t *__restrict__ src, int nsamp, uint32_t fill, uint32_t window, int thresh, int hold,
                                                            const gpsiq_agc_state_t *__restrict__ st_in, gpsiq_agc_state_t *__restrict__ st_out,
                                                            unsigned long long *__restrict__ wsum, uint32_t *__restrict__ wcnt, uint8_t *__restrict__ mask,
                                                            unsigned long long *__restrict__ blanked)
{
    constexpr int WAVES = kAgcThreads / 64;
    __shared__ unsigned long long s_sum[kAgcTileWindows + 1];
    __shared__ uint32_t s_cnt[kAgcTileWindows + 1];
    __shared__ int s_lead[WAVES], s_wave[WAVES];
    __shared__ uint32_t s_blank[WAVES];
    const int tid = (int) threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t t0 = (uint64_t) blockIdx.x * kAgcTile;
    const uint64_t hold_in = st_in->hold;
    if (tid <= kAgcTileWindows) { s_sum[tid] = 0; s_cnt[tid] = 0; }
    const uint64_t m0 = t0 + (uint64_t) tid * kAgcUnit;
    const int n = m0 >= (uint64_t) nsamp ? 0 : (uint64_t) nsamp - m0 < (uint64_t) kAgcUnit ? (int) ((uint64_t) nsamp - m0) : kAgcUnit;
    int x[2 * kAgcUnit];
    load_unit<FMT>(src, m0, n, x);
    uint32_t ebits = 0;
    int last = kNone, lead_last = kNone;       // sample indices relative to the tile's first sample
    if (MASK) {
        ebits = exceed_bits(x, thresh);
        // the lead-in: the units that hold the `hold` samples in front of the tile, all of them inside the span
        const int lead_units = (hold + kAgcUnit - 1) / kAgcUnit;
        int mine = kNone;
        if (tid < lead_units) {
            const int64_t lu = (int64_t) (t0 / kAgcUnit) - lead_units + tid;
            if (lu >= 0) {
                int y[2 * kAgcUnit];
                load_unit<FMT>(src, (uint64_t) lu * kAgcUnit, kAgcUnit, y);
                const uint32_t eb = exceed_bits(y, thresh);
                if (eb) mine = (tid - lead_units) * kAgcUnit + 31 - __clz(eb);
            }
        }
        mine = wave_max(mine);
        if (lane == 0) s_lead[wave] = mine;
        // the last exceeding sample of the units up to this one: an inclusive prefix maximum over the wave ...
        int inc = ebits ? tid * kAgcUnit + 31 - __clz(ebits) : kNone;
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(inc, off, 64);
            if (lane >= off && o > inc) inc = o;
        }
        if (lane == 63) s_wave[wave] = inc;
        last = __shfl_up(inc, 1, 64);
        if (lane == 0) last = kNone;
    }
    __syncthreads();
    if (MASK) {
        // ... and over the lead-in and the waves before
#pragma unroll
        for (int k = 0; k < WAVES; ++k) lead_last = s_lead[k] > lead_last ? s_lead[k] : lead_last;
        last = lead_last > last ? lead_last : last;
        for (int k = 0; k < wave; ++k) last = s_wave[k] > last ? s_wave[k] : last;
    }
    // the unit's samples in order: blank flags, and the power of the unblanked ones in the window they belong to.  Sample j lies in
    // window wi0 while j < rem, in wi0 + 1 from there on (a window has at least 64 samples)
    const uint32_t pos = fill + (uint32_t) m0;
    const uint32_t wi0 = pos / window, rem = window - (pos - wi0 * window);
    unsigned long long a0 = 0, a1 = 0;
    uint32_t c0 = 0, c1 = 0, bbits = 0;
#pragma unroll
    for (int j = 0; j < kAgcUnit; ++j) {
        if (j >= n) continue;
        bool b = m0 + (uint64_t) j < hold_in;
        if (MASK) {
            const int at = tid * kAgcUnit + j;
            if ((ebits >> j) & 1u) last = at;
            b = b || last >= at - hold;
        }
        if (b) bbits |= 1u << j;
        else {
            const uint32_t sq = (uint32_t) (x[2 * j] * x[2 * j]) + (uint32_t) (x[2 * j + 1] * x[2 * j + 1]);      // at most 2^31
            if ((uint32_t) j < rem) { a0 += sq; c0 += 2; } else { a1 += sq; c1 += 2; }
        }
    }
    if (MASK && n > 0) mask[m0 / kAgcUnit] = (uint8_t) bbits;
    // per wave where the wave's samples share a window, else per lane; then per workgroup in LDS
    const uint32_t wt0 = (fill + (uint32_t) t0) / window;
    const uint32_t wf = (uint32_t) __shfl((int) wi0, 0, 64);
    if (__all(n == 0 || (wi0 == wf && rem >= (uint32_t) n))) {
        for (int off = 32; off >= 1; off >>= 1) { a0 += __shfl_xor(a0, off, 64); c0 += __shfl_xor(c0, off, 64); }
        if (lane == 0 && c0) { atomicAdd(&s_sum[wf - wt0], a0); atomicAdd(&s_cnt[wf - wt0], c0); }
    } else {
        if (c0) { atomicAdd(&s_sum[wi0 - wt0], a0); atomicAdd(&s_cnt[wi0 - wt0], c0); }
        if (c1) { atomicAdd(&s_sum[wi0 - wt0 + 1], a1); atomicAdd(&s_cnt[wi0 - wt0 + 1], c1); }
    }
    uint32_t nb = (uint32_t) __popc(bbits);
    for (int off = 32; off >= 1; off >>= 1) nb += __shfl_xor(nb, off, 64);
    if (lane == 0) s_blank[wave] = nb;
    __syncthreads();
    // one atomic pair per workgroup and window that counted anything (a window with a count lies inside the span's nwin)
    if (tid <= kAgcTileWindows && s_cnt[tid]) {
        atomicAdd(&wsum[(size_t) wt0 + tid], s_sum[tid]);
        atomicAdd(&wcnt[(size_t) wt0 + tid], s_cnt[tid]);
    }
    if (tid == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) sum += s_blank[k];
        if (sum) atomicAdd(blanked, sum);
        if (MASK && blockIdx.x == gridDim.x - 1) {
            // the hold the span leaves: what is left of the one handed in, and what the last exceeding sample still covers
            int e_last = lead_last;
#pragma unroll
            for (int k = 0; k < WAVES; ++k) e_last = s_wave[k] > e_last ? s_wave[k] : e_last;
            const int64_t behind = (int64_t) nsamp - (int64_t) t0 - 1 - (int64_t) e_last;
            int64_t h = (int64_t) hold - behind;
            const int64_t left = (int64_t) hold_in - (int64_t) nsamp;
            h = left > h ? left : h;
            st_out->hold = h > 0 ? (uint32_t) h : 0u;
        }
    }
}

// Arguments: gpsiq_agc.h.  Window j of the span in total: its slot, and for the span's first window what the state held of it.
__global__ __launch_bounds__(kAgcThreads) void agc_gains(uint32_t nwin, int nsamp, uint32_t fill, uint32_t window, AgcGain g, int hold_written,
                                                          const gpsiq_agc_state_t *__restrict__ st_in, gpsiq_agc_state_t *__restrict__ st_out,
                                                          const unsigned long long *__restrict__ wsum, const uint32_t *__restrict__ wcnt,
                                                          uint32_t *__restrict__ mults)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kAgcThreads + tid;
    const int64_t nring = (int64_t) st_in->nring;
    if (i < nwin) {
        // the ring at the window's start: the navg complete windows before it, of the span first, then of the state
        unsigned long long S = 0, n = 0;
        for (int k = 1; k <= g.navg; ++k) {
            const int64_t j = (int64_t) i - k;
            if (j >= 0) {
                S += wsum[j] + (j == 0 ? st_in->psum : 0ull);
                n += wcnt[j] + (j == 0 ? st_in->pcnt : 0u);
            } else {
                const int64_t r = nring + j;
                if (r < 0) break;
                S += st_in->wsum[r];
                n += st_in->wcnt[r];
            }
        }
        mults[i] = agc_gain(S, n, g.target_q8, g.mult0, g.mult_min, g.mult_max);
    }
    if (blockIdx.x == 0 && tid < (uint32_t) kAgcMaxAvg) {
        const uint64_t end = (uint64_t) fill + (uint64_t) (uint32_t) nsamp;
        const uint64_t ncomp = end / window;
        const uint32_t nfill = (uint32_t) (end - ncomp * window);
        const uint64_t have = (uint64_t) nring + ncomp;
        const uint32_t keep = have < (uint64_t) g.navg ? (uint32_t) have : (uint32_t) g.navg;
        unsigned long long s = 0;
        uint32_t c = 0;
        if (tid < keep) {                      // entry tid of the ring: the last `keep` of [the state's ring | the span's complete windows]
            const uint64_t q = have - keep + tid;
            if (q < (uint64_t) nring) { s = st_in->wsum[q]; c = st_in->wcnt[q]; }
            else {
                const uint64_t j = q - (uint64_t) nring;
                s = wsum[j] + (j == 0 ? st_in->psum : 0ull);
                c = wcnt[j] + (j == 0 ? st_in->pcnt : 0u);
            }
        }
        st_out->wsum[tid] = s;
        st_out->wcnt[tid] = c;
        if (tid == 0) {
            st_out->psum = nfill ? wsum[ncomp] + (ncomp == 0 ? st_in->psum : 0ull) : 0ull;
            st_out->pcnt = nfill ? wcnt[ncomp] + (ncomp == 0 ? st_in->pcnt : 0u) : 0u;
            st_out->fill = nfill;
            st_out->nring = keep;
            if (!hold_written) st_out->hold = st_in->hold > (uint32_t) nsamp ? st_in->hold - (uint32_t) nsamp : 0u;
        }
    }
}

// Arguments: gpsiq_agc.h.  Lane t of workgroup w has units (w * kAgcApplyUnits + k) * kAgcThreads + t: the loads of a step are
// contiguous over the workgroup.
template <int FMT, int OFMT, bool MASK>
__global__ __launch_bounds__(kAgcThreads) void agc_apply(const uint8_t *__restrict__ src, int nsamp, uint32_t fill, uint32_t window,
                                                          const uint32_t *__restrict__ mults, const uint8_t *__restrict__ mask,
                                                          const gpsiq_agc_state_t *__restrict__ st_in, int qmax, uint8_t *__restrict__ dst, uint32_t units,
                                                          unsigned long long *__restrict__ count)
{
    const uint64_t hold_in = st_in->hold;
    unsigned long long clipped = 0;
#pragma unroll
    for (int k = 0; k < kAgcApplyUnits; ++k) {
        const uint64_t u = ((uint64_t) blockIdx.x * kAgcApplyUnits + k) * kAgcThreads + threadIdx.x;
        if (u >= units) continue;
        const uint64_t m0 = u * kAgcUnit;
        const int n = (uint64_t) nsamp - m0 < (uint64_t) kAgcUnit ? (int) ((uint64_t) nsamp - m0) : kAgcUnit;
        int x[2 * kAgcUnit];
        load_unit<FMT>(src, m0, n, x);
        const uint32_t pos = fill + (uint32_t) m0;
        const uint32_t wi0 = pos / window, rem = window - (pos - wi0 * window);
        const uint32_t g0 = mults[wi0], g1 = rem < (uint32_t) n ? mults[wi0 + 1] : 0u;
        const uint32_t bbits = MASK ? mask[u] : 0u;
        int y[2 * kAgcUnit];
#pragma unroll
        for (int j = 0; j < kAgcUnit; ++j) {
            const bool b = MASK ? ((bbits >> j) & 1u) != 0 : m0 + (uint64_t) j < hold_in;
            const long long g = (uint32_t) j < rem ? g0 : g1;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long v = ((long long) x[2 * j + c] * g + 32768) >> 16;
                const int o = v < -qmax ? -qmax : v > qmax ? qmax : (int) v;
                y[2 * j + c] = b ? 0 : o;
                clipped += !b && (long long) o != v;           // (elements past the span read as zeros: never clamped)
            }
        }
        if (n == kAgcUnit) {                                   // all of the unit is the span's: so are its destination bytes
            if (OFMT == GPSIQ_SC08) {
                Quad q;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    q.w[e] = ((uint32_t) y[4 * e] & 0xffu) | (((uint32_t) y[4 * e + 1] & 0xffu) << 8) | (((uint32_t) y[4 * e + 2] & 0xffu) << 16) |
                             ((uint32_t) y[4 * e + 3] << 24);
                store16(dst + m0 * 2, q);
            } else {
                Quad a, b2;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a.w[e] = ((uint32_t) y[2 * e] & 0xffffu) | ((uint32_t) y[2 * e + 1] << 16);
                    b2.w[e] = ((uint32_t) y[8 + 2 * e] & 0xffffu) | ((uint32_t) y[8 + 2 * e + 1] << 16);
                }
                store16(dst + m0 * 4, a);
                store16(dst + m0 * 4 + 16, b2);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 2 * kAgcUnit; ++e) {
                if (e >= 2 * n) continue;
                if (OFMT == GPSIQ_SC16) reinterpret_cast<int16_t *>(dst)[2 * m0 + e] = (int16_t) y[e];
                else reinterpret_cast<int8_t *>(dst)[2 * m0 + e] = (int8_t) y[e];
            }
        }
    }
    // count_clipped's steps (gpsiq_stream.h), kept in place: calling the shared one changes this kernel's code object
    for (int off = 32; off >= 1; off >>= 1) clipped += __shfl_xor(clipped, off, 64);
    __shared__ unsigned long long part[kAgcThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = clipped;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < kAgcThreads / 64; ++k) sum += part[k];
        if (sum) atomicAdd(count, sum);
    }
}

template <int FMT, bool MASK>
AgcApplyFn apply_to(int out_fmt)
{
    return out_fmt == GPSIQ_SC08 ? agc_apply<FMT, GPSIQ_SC08, MASK> : out_fmt == GPSIQ_SC16 ? agc_apply<FMT, GPSIQ_SC16, MASK> : nullptr;
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_agc.cpp looks up.  nullptr: no such kernel.
AgcMeasureFn agc_measure_kernel(int in_fmt, bool mask)
{
    if (in_fmt == GPSIQ_SC08) return mask ? agc_measure<GPSIQ_SC08, true> : agc_measure<GPSIQ_SC08, false>;
    if (in_fmt == GPSIQ_SC16) return mask ? agc_measure<GPSIQ_SC16, true> : agc_measure<GPSIQ_SC16, false>;
    return nullptr;
}

AgcGainsFn agc_gains_kernel() { return agc_gains; }

AgcApplyFn agc_apply_kernel(int in_fmt, int out_fmt, bool mask)
{
    if (in_fmt == GPSIQ_SC08) return mask ? apply_to<GPSIQ_SC08, true>(out_fmt) : apply_to<GPSIQ_SC08, false>(out_fmt);
    if (in_fmt == GPSIQ_SC16) return mask ? apply_to<GPSIQ_SC16, true>(out_fmt) : apply_to<GPSIQ_SC16, false>(out_fmt);
    return nullptr;
}
}  // namespace gpsiq
