// gpsiq_mix_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_mix (include/gpsiq_rows.h, "Mix"): up to eight terms -- a stream as
// it is, a stream rotated by an NCO over the 512-entry carrier table, the bare NCO -- each gated, delayed and scaled by an integer gain,
// summed in int64, rounded, clamped and counted.
//   mix_generic<OUT>   every kind, every source format, any alignment: a thread takes one complex sample and evaluates every term's
//                      gate, sweep position and phase from the closed form of the contract
//   mix_rows<OUT>      a lane owns a SLOT, 16 aligned bytes of dst (gpsiq_mix_geometry.h): it evaluates the closed form at the slot's
//                      first sample and steps it from there, reads a source run in the widest loads its address allows and writes the
//                      slot in one 16-byte store; the first and the last slot of a span may be partial and go sample by sample
// Stepping is exact: with base = phase0 + m step and sw = tri(r) rate, the phase is base + sw (mod 2^59); one sample on, base grows by
// step and sw by r rate (tri(r + 1) - tri(r) = r), and where the sweep restarts r and sw are 0 again.  All in wrapping uint64, of which
// 2^59 is a divisor.  The host sends a span to mix_rows only where neither m nor m + offset wraps inside it (gpsiq_mix_plan.h).
// The accumulator cannot wrap: |x| <= 2^15, |c|, |s| <= 250, so |t| <= 2^15 * 500 < 2^24; |gain| <= 2^31; eight terms: < 2^58; the
// rounding constant is at most 2^39.
// In place: dst may be the src of one stream term with skip 0 and dst's format.  Both kernels read every source sample of an output
// before they write it, and no thread reads an element another thread writes (the host refuses every other overlap): in mix_generic
// a thread reads sample n of that term and writes sample n, in mix_rows a lane reads the very slot it writes.  Hence no __restrict__
// on dst.  Every offset into a source or dst is 64 bits wide.  Sample n - skip of a source is read only for skip <= n < nsamp; dst is
// written for samples 0 <= n < nsamp and nowhere else.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_mix_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

typedef uint32_t mix_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mix_u32x2 __attribute__((ext_vector_type(2)));

// r (r - 1) / 2 mod 2^64: the even factor is halved before the product
__device__ __forceinline__ uint64_t mix_tri(uint64_t r) { return (r & 1) ? r * ((r - 1) >> 1) : (r >> 1) * (r - 1); }

// a term's gate position, sweep position and the two parts of its phase at one absolute sample
struct MixNco {
    uint64_t base, sw, r;
    uint32_t g;
};

__device__ __forceinline__ MixNco nco_at(const MixDevTerm &t, uint64_t m)
{
    MixNco s;
    s.r = t.sweep_period ? (m + t.sweep_offset) % t.sweep_period : m;
    s.base = t.phase0 + m * t.step;
    s.sw = mix_tri(s.r) * t.rate;
    s.g = t.gate_period ? (uint32_t) ((m + t.gate_offset) % t.gate_period) : 0u;
    return s;
}

__device__ __forceinline__ void nco_step(const MixDevTerm &t, MixNco &s)
{
    s.base += t.step;
    s.sw += s.r * t.rate;
    ++s.r;
    if (t.sweep_period && s.r == t.sweep_period) { s.r = 0; s.sw = 0; }
    if (t.gate_period && ++s.g == t.gate_period) s.g = 0;
}

__device__ __forceinline__ bool nco_on(const MixDevTerm &t, const MixNco &s) { return !t.gate_period || s.g < t.gate_on; }

// gain * t of one term into the sums; tab: the table in LDS, cos in the low half of a word, sin in the high half
__device__ __forceinline__ void add_term(const MixDevTerm &t, const MixNco &s, const uint32_t *tab, int xi, int xq, long long &ai, long long &aq)
{
    int ti = xi, tq = xq;
    if (t.kind != GPSIQ_MIX_STREAM) {
        const uint32_t w = tab[(uint32_t) ((s.base + s.sw) >> 50) & 511u];
        const int c = (int) (int16_t) (w & 0xffffu), sn = (int32_t) w >> 16;
        if (t.kind == GPSIQ_MIX_TONE) { ti = c; tq = sn; }
        else { ti = xi * c - xq * sn; tq = xi * sn + xq * c; }
    }
    ai += (long long) t.gain * ti;
    aq += (long long) t.gain * tq;
}

// sample j of a source, I and Q sign-extended
__device__ __forceinline__ void load_one(const uint8_t *src, int fmt, uint64_t j, int &xi, int &xq)
{
    if (fmt == GPSIQ_SC16) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(src + j * 4);
        xi = (int) (int16_t) (v & 0xffffu);
        xq = (int32_t) v >> 16;
    } else {
        const uint32_t v = *reinterpret_cast<const uint16_t *>(src + j * 2);
        xi = (int) (int8_t) (v & 0xffu);
        xq = (int) (int8_t) (v >> 8);
    }
}

// y = floor((acc + 2^(shift-1)) / 2^shift), clamped to +-qmax; clipped counts the elements the clamp changed
__device__ __forceinline__ int finish(long long acc, int shift, int qmax, unsigned &clipped)
{
    const long long half = shift ? (long long) 1 << (shift - 1) : 0;
    const long long y = (acc + half) >> shift;
    const long long c = y < -(long long) qmax ? -(long long) qmax : y > (long long) qmax ? (long long) qmax : y;
    clipped += c != y;
    return (int) c;
}

using stream::store_sample;
using stream::count_clipped;

// Arguments: the terms, m0, the samples, shift, qmax, the destination, the table as 512 dwords (cos in the low half, sin in the high
// half), the counter (zeroed by the host).  Thread t of the launch takes samples t, t + gridDim.x * kMixThreads, ...
template <int OUT>
__global__ __launch_bounds__(kMixThreads) void mix_generic(const MixDevTerms terms, uint64_t m0, int nsamp, int shift, int qmax, uint8_t *dst,
                                                           const uint32_t *__restrict__ table, unsigned long long *__restrict__ count)
{
    __shared__ uint32_t tab[512];
    for (int i = threadIdx.x; i < 512; i += kMixThreads) tab[i] = table[i];
    __syncthreads();
    unsigned clipped = 0;
    const uint64_t stride = (uint64_t) gridDim.x * kMixThreads;
    for (uint64_t n = (uint64_t) blockIdx.x * kMixThreads + threadIdx.x; n < (uint64_t) nsamp; n += stride) {
        long long ai = 0, aq = 0;
        for (int k = 0; k < terms.n; ++k) {
            const MixDevTerm &t = terms.t[k];
            const MixNco s = nco_at(t, m0 + n);
            if (!nco_on(t, s)) continue;
            int xi = 0, xq = 0;
            if (t.kind != GPSIQ_MIX_TONE) {
                if (n < t.skip) continue;                                  // zeros before the delay
                load_one(t.src, t.fmt, n - t.skip, xi, xq);
            }
            add_term(t, s, tab, xi, xq, ai, aq);
        }
        store_sample<OUT>(dst, n, finish(ai, shift, qmax, clipped), finish(aq, shift, qmax, clipped));
    }
    count_clipped<kMixThreads>(clipped, count);
}

// S whole samples of a source at p: dword loads where p is 4-byte aligned (always for int16; for int8 unless the delay is odd), as
// one or two 16-byte loads (8 bytes for four int8 samples) where p is aligned to that too
template <int FMT, int S>
__device__ __forceinline__ void load_full(const uint8_t *p, int *xi, int *xq)
{
    constexpr int W = S * 2 * FMT / 4;                                     // dwords of the run: 2, 4 or 8
    const uintptr_t a = (uintptr_t) p;
    if (FMT == GPSIQ_SC08 && (a & 3)) {
#pragma unroll
        for (int i = 0; i < S; ++i) load_one(p, FMT, (uint64_t) i, xi[i], xq[i]);
        return;
    }
    uint32_t w[W];
    if (W >= 4 && !(a & 15)) {
#pragma unroll
        for (int j = 0; j < W / 4; ++j) {
            const mix_u32x4 v = reinterpret_cast<const mix_u32x4 *>(p)[j];
            w[4 * j] = v[0]; w[4 * j + 1] = v[1]; w[4 * j + 2] = v[2]; w[4 * j + 3] = v[3];
        }
    } else if (W == 2 && !(a & 7)) {
        const mix_u32x2 v = *reinterpret_cast<const mix_u32x2 *>(p);
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

// x(n0 + i) of a stream term for the slot positions lo <= i < hi (the others stay 0): false if every one of them is a zero before the
// delay.  Nothing but samples skip <= n < nsamp of the contract is read: a run that is whole and past the delay goes to load_full,
// every other one sample by sample.
template <int FMT, int S>
__device__ __forceinline__ bool load_run(const MixDevTerm &t, int64_t n0, int lo, int hi, int *xi, int *xq)
{
#pragma unroll
    for (int i = 0; i < S; ++i) { xi[i] = 0; xq[i] = 0; }
    const int64_t sk = t.skip > (uint64_t) INT32_MAX ? (int64_t) INT32_MAX : (int64_t) t.skip;     // (n0 + hi <= nsamp <= INT32_MAX)
    if (n0 + hi <= sk) return false;
    const int64_t f = n0 - sk;                                             // the source sample at slot position 0
    if (lo == 0 && hi == S && f >= 0) {
        load_full<FMT, S>(t.src + (uint64_t) f * (2 * FMT), xi, xq);
        return true;
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
        if (i >= lo && i < hi && f + i >= 0) load_one(t.src, FMT, (uint64_t) (f + i), xi[i], xq[i]);
    return true;
}

// Arguments: the terms, m0, the samples, shift, qmax, the destination, the samples of the first slot that lie before sample 0, the
// slots of the launch (gpsiq_mix_plan.h), the table, the counter (zeroed by the host).  Slot u holds samples u S - lead .. u S - lead
// + S - 1, those of them in [0, nsamp); its first byte is 16-byte aligned.  Thread t of the launch takes slots t, t + gridDim.x *
// kMixThreads, ...: the lanes of a wave write 1 KiB back to back.
template <int OUT>
__global__ __launch_bounds__(kMixThreads) void mix_rows(const MixDevTerms terms, uint64_t m0, int nsamp, int shift, int qmax, uint8_t *dst, int lead,
                                                        uint64_t slots, const uint32_t *__restrict__ table, unsigned long long *__restrict__ count)
{
    constexpr int S = mix_slot_samples(OUT);
    __shared__ uint32_t tab[512];
    for (int i = threadIdx.x; i < 512; i += kMixThreads) tab[i] = table[i];
    __syncthreads();
    unsigned clipped = 0;
    const uint64_t stride = (uint64_t) gridDim.x * kMixThreads;
    for (uint64_t u = (uint64_t) blockIdx.x * kMixThreads + threadIdx.x; u < slots; u += stride) {
        const int64_t n0 = (int64_t) u * S - lead;
        const int lo = n0 < 0 ? (int) -n0 : 0;
        const int64_t left = (int64_t) nsamp - n0;
        const int hi = left < S ? (int) left : S;
        long long ai[S], aq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) { ai[i] = 0; aq[i] = 0; }
        for (int k = 0; k < terms.n; ++k) {
            const MixDevTerm &t = terms.t[k];
            int xi[S], xq[S];
            if (t.kind != GPSIQ_MIX_TONE) {
                const bool any = t.fmt == GPSIQ_SC16 ? load_run<GPSIQ_SC16, S>(t, n0, lo, hi, xi, xq) : load_run<GPSIQ_SC08, S>(t, n0, lo, hi, xi, xq);
                if (!any) continue;
            } else {
#pragma unroll
                for (int i = 0; i < S; ++i) { xi[i] = 0; xq[i] = 0; }
            }
            MixNco s = nco_at(t, m0 + (uint64_t) (n0 + lo));              // the slot's first sample that exists
#pragma unroll
            for (int i = 0; i < S; ++i) {
                if (i >= lo && i < hi) {
                    // (a stream sample before the delay is a zero: gain * 0, rotated or not)
                    if (nco_on(t, s)) add_term(t, s, tab, xi[i], xq[i], ai[i], aq[i]);
                    nco_step(t, s);
                }
            }
        }
        int oi[S], oq[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            oi[i] = finish(ai[i], shift, qmax, clipped);
            oq[i] = finish(aq[i], shift, qmax, clipped);
        }
        if (lo == 0 && hi == S) {
            mix_u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (OUT == GPSIQ_SC16) v[j] = ((uint32_t) oi[j] & 0xffffu) | ((uint32_t) oq[j] << 16);
                else v[j] = ((uint32_t) oi[2 * j] & 0xffu) | (((uint32_t) oq[2 * j] & 0xffu) << 8) | (((uint32_t) oi[2 * j + 1] & 0xffu) << 16) |
                            ((uint32_t) oq[2 * j + 1] << 24);
            }
            *reinterpret_cast<mix_u32x4 *>(dst + (uint64_t) n0 * (2 * OUT)) = v;
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i)
                if (i >= lo && i < hi) store_sample<OUT>(dst, (uint64_t) (n0 + i), oi[i], oq[i]);
        }
    }
    count_clipped<kMixThreads>(clipped, count);
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_mix.cpp looks up.  nullptr: no such kernel.
MixGenericFn mix_generic_kernel(int out_fmt)
{
    return out_fmt == GPSIQ_SC08 ? mix_generic<GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? mix_generic<GPSIQ_SC16> : nullptr;
}

MixRowsFn mix_rows_kernel(int out_fmt) { return out_fmt == GPSIQ_SC08 ? mix_rows<GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? mix_rows<GPSIQ_SC16> : nullptr; }
}  // namespace gpsiq
