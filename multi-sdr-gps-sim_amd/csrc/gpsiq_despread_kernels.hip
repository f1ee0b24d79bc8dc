// gpsiq_despread_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_despread (include/gpsiq_rows.h, "Despread"): the
// receiver's first stage run over a rendered stream.  For every active channel of a block the stream is multiplied by the conjugate
// of the channel's replica -- the closed form of include/gpsiq.h for that channel alone with gain 1.0, data bit included -- and
// summed over segments.  Everything is integer arithmetic, so the sums are a pure function of (descriptors, stream bytes) and the
// order in which partial sums meet does not matter: waves add theirs with 64-bit integer atomics into outputs the host has zeroed.
//   despread_generic   one sample per lane per step, every quantity of the closed form at full width (any rate): the fallback for
//                      sample rates too low for the row kernel, and the second implementation the tests hold the row kernel against
//   despread_rows      the synthesis row loop run backwards: a row is 64 consecutive samples, a wave owns a run of rows, per channel
//                      two 64-bit NCO words per lane and one 32-chip sign window per row (gpsiq_signal.h)
// The replica comes from ONE unit table for all channels (512 entries, cos | sin << 16, 2 KB of LDS).  No MFMA: per sample and
// channel the work is one 2x2 integer rotation, two v_dot2_i32_i16.
#include <hip/hip_runtime.h>

#include <array>

#include "gpsiq_ctx.h"
#include "gpsiq_despread_geometry.h"
#include "gpsiq_signal.h"

namespace gpsiq {
namespace {

constexpr int kDsMaxChan = GPSIQ_MAX_CHAN;
constexpr int kDsThreads = kDespreadWaves * 64;

typedef short ds_s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void atomic_add_i64(int64_t *p, int64_t v)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long) v);      // two's complement: the same addition
}

// the stream's own statistics, from the load the correlator makes anyway.  Per lane in 64 bits for the wave's whole run.
struct LaneStats {
    int64_t  si = 0, sq = 0;
    uint64_t qi = 0, qq = 0;
    uint32_t ci = 0, cq = 0;
    __device__ __forceinline__ void add(int i, int q, bool valid, int clip)
    {
        si += i; sq += q;
        qi += (uint64_t) ((int64_t) i * i); qq += (uint64_t) ((int64_t) q * q);
        ci += valid && (i < 0 ? -i : i) >= clip; cq += valid && (q < 0 ? -q : q) >= clip;
    }
    // every lane of the wave calls it
    __device__ __forceinline__ void flush(gpsiq_block_stats_t *st, int lane)
    {
        const int64_t a = wave_sum(si), b = wave_sum(sq), c = wave_sum((int64_t) qi), d = wave_sum((int64_t) qq);
        const int64_t e = wave_sum((int64_t) (((uint64_t) cq << 32) | ci));      // two 32-bit counts, each < 2^32 over a block
        if (lane == 0) {
            atomic_add_i64(&st->sum_i, a); atomic_add_i64(&st->sum_q, b);
            atomic_add_i64(reinterpret_cast<int64_t *>(&st->sumsq_i), c); atomic_add_i64(reinterpret_cast<int64_t *>(&st->sumsq_q), d);
            atomicAdd(&st->clip_i, (uint32_t) e); atomicAdd(&st->clip_q, (uint32_t) ((uint64_t) e >> 32));
        }
    }
};

}  // namespace

// ---------------------------------------------------------------------------
// Generic kernel.  A wave owns wave_rows consecutive rows of its block; channel by channel it walks them with the closed form at
// full width per sample and a 64-bit sum per lane, which the wave adds up and hands over at every segment edge and at the end of
// its run.  The stream is read once per channel (and once for the statistics): this is the fallback, not the fast path.
template <int FMT>
__global__ __launch_bounds__(kDsThreads) void despread_generic(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, const uint8_t *__restrict__ src, size_t block_stride, int block0,
    const DeviceTables *__restrict__ tab, int tiles_per_block, int wave_rows, int seg_rows, int nseg, int clip,
    gpsiq_despread_sum_t *__restrict__ sums, uint8_t *__restrict__ prn_out, gpsiq_block_stats_t *__restrict__ stats)
{
    __shared__ uint32_t unit[512];
    __shared__ uint32_t ext[kDsMaxChan][kPrnExtWords];
    __shared__ gpsiq_qchan_t qs[kDsMaxChan];

    const int tid = threadIdx.x;
    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    const gpsiq_qchan_t *q_blk = desc + (size_t) (block0 + blk) * nchan;
    for (int i = tid; i < nchan * 12; i += kDsThreads)
        reinterpret_cast<uint32_t *>(qs)[i] = reinterpret_cast<const uint32_t *>(q_blk)[i];
    __syncthreads();
    stage_unit<kDsThreads>(tab, unit);
    for (int e = tid; e < nchan * kPrnExtWords; e += kDsThreads) {
        const int c = e / kPrnExtWords, w = e % kPrnExtWords;
        ext[c][w] = qs[c].prn ? tab->prn_ext[qs[c].prn - 1][w] : 0u;
    }
    if (tile == 0 && tid < nchan) prn_out[(size_t) blk * nchan + tid] = qs[tid].prn;
    __syncthreads();
    const uint8_t *blk_src = src + (size_t) blk * block_stride;

    const int wave = tid >> 6, lane = tid & 63;
    const int rows_total = (int) (((uint32_t) nsamp + 63u) >> 6);
    const int row_first = (tile * kDespreadWaves + wave) * wave_rows;
    if (row_first >= rows_total) return;                 // the whole wave: nothing below divides a wave
    const int rows = rows_total - row_first < wave_rows ? rows_total - row_first : wave_rows;
    const uint32_t n0 = (uint32_t) row_first * 64u + (uint32_t) lane;

    if (stats) {
        LaneStats st;
        for (int r = 0; r < rows; ++r) {
            const uint32_t n = n0 + (uint32_t) r * 64u;
            int si, sq;
            load_iq<FMT>(blk_src, n, &si, &sq, n < (uint32_t) nsamp);
            st.add(si, sq, n < (uint32_t) nsamp, clip);
        }
        st.flush(stats + blk, lane);
    }
    for (int c = 0; c < nchan; ++c) {
        const gpsiq_qchan_t &q = qs[c];
        if (q.prn == 0) continue;
        gpsiq_despread_sum_t *out = sums + ((size_t) blk * nchan + c) * nseg;
        int64_t ai = 0, aq = 0;
        int j = row_first / seg_rows, left = seg_rows - row_first % seg_rows;     // the segment of the row, rows left in it
        for (int r = 0; r < rows; ++r) {
            const uint32_t n = n0 + (uint32_t) r * 64u;
            int si, sq;
            load_iq<FMT>(blk_src, n, &si, &sq, n < (uint32_t) nsamp);
            const uint32_t idx = carrier_index(q, n);
            const uint64_t A = chip_count(q, n);
            const uint32_t chip = code_chip(A), bit = data_bit(q, A);
            const uint32_t neg = ((ext[c][chip >> 5] >> (chip & 31)) ^ (q.nav_bits >> (bit & 31))) & 1u;
            const uint32_t v = unit[idx];
            const int tc = (int16_t) (v & 0xffffu), ts = (int32_t) v >> 16;
            const int ri = neg ? -tc : tc, rq = neg ? -ts : ts;
            ai += si * ri + sq * rq;                       // each product below 2^23
            aq += sq * ri - si * rq;
            if (--left == 0 || r == rows - 1) {            // wave-uniform
                const int64_t ti = wave_sum(ai), tq = wave_sum(aq);
                if (lane == 0) { atomic_add_i64(&out[j].i, ti); atomic_add_i64(&out[j].q, tq); }
                ai = aq = 0;
                if (left == 0) { ++j; left = seg_rows; }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Row kernel.  Rows, NCO words and sign windows are those of the synthesis row kernels (gpsiq_signal.h); the windows are built
// kDespreadChunkRows rows at a time into LDS by the wave itself: lane (c, g) walks sixteen rows of channel c.
// Per row a lane loads its sample ONCE, takes the stream statistics from it and packs it twice, (I, Q) and (Q, I).  Per channel:
//   the sign enters as half a carrier cycle (the table is antisymmetric: entry k + 256 is minus entry k);
//   entry k is (cos, sin), entry 511 - k is (cos, -sin) (the table is a half-sample-offset sine: sin[511 - k] = -sin[k] and
//   cos[511 - k] = cos[k]), so both rotated components are one v_dot2_i32_i16 each, with no negation of a sample: -32768 is safe;
//   the terms go into two 32-bit per-lane partial sums.  One term is at most 2 * 32768 * 250 < 2^24 and the partials are widened
//   after kDespreadChunkRows = 64 rows at the latest, at every segment edge and at the end of the run: 64 x 2^24 < 2^31.
// Widening: eight partials at a time (in-phase, then quadrature, of eight channels) are summed over the 64 lanes by a transposing
// butterfly (step s: half of the values go to the partner lane, the other half come from it) in 64-bit arithmetic, after which
// eight lanes hold one total each and add it to the segment's output with one atomic.
template <int NV>
__device__ __forceinline__ int transpose_sum(int64_t (&v)[NV], int lane)
{
    static_assert(NV == 4 || NV == 8, "values per lane");
    int bit = 32;
#pragma unroll
    for (int n = NV; n > 1; n >>= 1, bit >>= 1) {
        const int half = n >> 1;
        const bool upper = (lane & bit) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const int64_t keep = upper ? v[i + half] : v[i], send = upper ? v[i] : v[i + half];
            v[i] = keep + __shfl_xor(send, bit, 64);
        }
    }
    for (; bit >= 1; bit >>= 1) v[0] += __shfl_xor(v[0], bit, 64);
    // lane L now holds the total of value L >> shift (every lane of a group of 1 << shift the same one)
    return NV == 8 ? 3 : 4;
}

// (Registers: the NCO words are 4 per channel, the partials 2, and the unrolled channel loop keeps its table reads in flight.  Up to
// eight slots fit the 128 registers of four waves per SIMD; twelve and sixteen would spill there and are compiled for two.)
template <int FMT, int NCH>
__global__ __launch_bounds__(kDsThreads, NCH <= 8 ? 4 : 2) void despread_rows(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, const uint8_t *__restrict__ src, size_t block_stride, int block0,
    const DeviceTables *__restrict__ tab, int tiles_per_block, int wave_rows, int seg_rows, int nseg, int clip,
    gpsiq_despread_sum_t *__restrict__ sums, uint8_t *__restrict__ prn_out, gpsiq_block_stats_t *__restrict__ stats)
{
    constexpr int CH = kDespreadChunkRows;
    constexpr int kRun = CH / 4;                          // rows one builder lane walks: four lane groups of sixteen channels
    constexpr int NV = NCH <= 4 ? 4 : 8;                  // partials widened at a time: a temporary of 2 * NV registers
    __shared__ uint32_t unit[512];
    __shared__ uint32_t ext[NCH][kPrnExtWords];
    __shared__ uint32_t win[kDespreadWaves][CH][NCH];
    __shared__ gpsiq_qchan_t qs[NCH];

    const int tid = threadIdx.x;
    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    const gpsiq_qchan_t *q_blk = desc + (size_t) (block0 + blk) * nchan;
    const int nq = nchan < NCH ? nchan : NCH;
    for (int i = tid; i < NCH * 12; i += kDsThreads)
        reinterpret_cast<uint32_t *>(qs)[i] = i < nq * 12 ? reinterpret_cast<const uint32_t *>(q_blk)[i] : 0u;
    __syncthreads();
    stage_unit<kDsThreads>(tab, unit);
    for (int e = tid; e < NCH * kPrnExtWords; e += kDsThreads) {
        const int c = e / kPrnExtWords, w = e % kPrnExtWords;
        ext[c][w] = qs[c].prn ? tab->prn_ext[qs[c].prn - 1][w] : 0u;
    }
    // (the descriptors are compacted, active channels first: slots past NCH are unused in every resident block)
    if (tile == 0 && tid < nchan) prn_out[(size_t) blk * nchan + tid] = tid < NCH ? qs[tid].prn : (uint8_t) 0;
    __syncthreads();
    const uint8_t *blk_src = src + (size_t) blk * block_stride;

    const int wave = tid >> 6, lane = tid & 63;
    const int rows_total = (int) (((uint32_t) nsamp + 63u) >> 6);
    const int row_first = (tile * kDespreadWaves + wave) * wave_rows;
    if (row_first >= rows_total) return;                 // the whole wave, behind the last workgroup barrier
    const int rows = rows_total - row_first < wave_rows ? rows_total - row_first : wave_rows;
    const uint32_t n0 = (uint32_t) row_first * 64u + (uint32_t) lane;

    // ---- per-lane NCO state of every channel (steps in SGPRs via scalar loads, as in the synthesis) -----
    uint64_t P[NCH], Q[NCH], dP[NCH], dQ[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        nco_start(q_blk, c, c < nchan, n0, &P[c], &Q[c], &dP[c], &dQ[c]);
    int32_t acc_i[NCH], acc_q[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc_i[c] = acc_q[c] = 0;
    LaneStats st;
    const unsigned char *unit_b = reinterpret_cast<const unsigned char *>(unit);
    int j = row_first / seg_rows, left = seg_rows - row_first % seg_rows;         // the segment of the row, rows left in it

    for (int row0 = 0; row0 < rows; row0 += CH) {
        // ---- windows of rows row0 .. row0 + CH - 1: lane (c, g) prepares rows g*kRun .. g*kRun + kRun - 1 of channel c ----
        {
            const int c = lane & 15, g = lane >> 4;
            if (c < NCH) {
                const gpsiq_qchan_t &q = qs[c];
                const bool on = q.prn != 0;
                const uint32_t n_row = (uint32_t) (row_first + row0 + g * kRun) * 64u;
#include "gpsiq_window_setup.inc"
#pragma unroll 4
                for (int r = 0; r < kRun; ++r) {
#include "gpsiq_window_row.inc"
                    win[wave][g * kRun + r][c] = on ? window_word(S, a5) : 0u;
#include "gpsiq_window_step.inc"
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");

        const int nr = rows - row0 < CH ? rows - row0 : CH;
        for (int r = 0; r < nr; ++r) {
            const uint32_t n = n0 + (uint32_t) (row0 + r) * 64u;
            const bool valid = n < (uint32_t) nsamp;
            int si, sq;
            load_iq<FMT>(blk_src, n, &si, &sq, valid);
            st.add(si, sq, valid, clip);
            const uint32_t iq = ((uint32_t) si & 0xffffu) | ((uint32_t) sq << 16);        // (I, Q)
            const uint32_t qi = __builtin_amdgcn_alignbit(iq, iq, 16u);                      // (Q, I)
            const uint32_t *w_row = win[wave][r];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const uint32_t t = w_row[c] >> ((uint32_t) (Q[c] >> 56) & 31u);           // bit 0 = chip ^ data bit of this lane
                const uint32_t x = (t << 26) + (uint32_t) (P[c] >> 32);                    // + half a cycle when that bit is set
                const uint32_t a = (x >> 16) & 0x7fcu;                                     // 4 * table index
                const uint32_t e1 = *reinterpret_cast<const uint32_t *>(unit_b + a);            // (rI, rQ)
                const uint32_t e2 = *reinterpret_cast<const uint32_t *>(unit_b + (a ^ 0x7fcu)); // (rI, -rQ)
                acc_i[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, iq), __builtin_bit_cast(ds_s16x2, e1), acc_i[c], false);
                acc_q[c] = __builtin_amdgcn_sdot2(__builtin_bit_cast(ds_s16x2, qi), __builtin_bit_cast(ds_s16x2, e2), acc_q[c], false);
                P[c] += dP[c];
                Q[c] += dQ[c];
            }
            if (--left == 0 || r == nr - 1) {                // wave-uniform: a segment edge, or the chunk (and maybe the run) ends
                gpsiq_despread_sum_t *out = sums + (size_t) blk * nchan * nseg + j;       // slot 0's segment j
#pragma unroll
                for (int pass = 0; pass < 2 * ((NCH + NV - 1) / NV); ++pass) {       // NV in-phase partials at a time, then the quadrature ones
                    const int comp = pass & 1, base = (pass >> 1) * NV;
                    int64_t v[NV];
#pragma unroll
                    for (int c = 0; c < NV; ++c) v[c] = base + c < NCH ? (int64_t) (comp ? acc_q : acc_i)[base + c < NCH ? base + c : 0] : 0;
                    const int shift = transpose_sum<NV>(v, lane);
                    const int c = base + (lane >> shift);
                    if ((lane & ((1 << shift) - 1)) == 0 && c < nq && qs[c].prn != 0)
                        atomic_add_i64(comp ? &out[(size_t) c * nseg].q : &out[(size_t) c * nseg].i, v[0]);
                }
#pragma unroll
                for (int c2 = 0; c2 < NCH; ++c2) acc_i[c2] = acc_q[c2] = 0;
                if (left == 0) { ++j; left = seg_rows; }
            }
        }
        // the next chunk overwrites this wave's windows: all lanes must be done reading
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (stats) st.flush(stats + blk, lane);
}

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_despread.cpp looks up with the values of a plan (gpsiq_despread_plan.h).
// slots is ignored for the generic kernel; nullptr: no such kernel.
DespreadFn despread_kernel(int fmt, int kernel, int slots)
{
    if (fmt != GPSIQ_SC08 && fmt != GPSIQ_SC16) return nullptr;
    const bool w = fmt == GPSIQ_SC16;
    if (kernel == 0) return w ? despread_generic<GPSIQ_SC16> : despread_generic<GPSIQ_SC08>;
    if (kernel != 1) return nullptr;
    switch (slots) {
    case 4:  return w ? despread_rows<GPSIQ_SC16, 4> : despread_rows<GPSIQ_SC08, 4>;
    case 8:  return w ? despread_rows<GPSIQ_SC16, 8> : despread_rows<GPSIQ_SC08, 8>;
    case 12: return w ? despread_rows<GPSIQ_SC16, 12> : despread_rows<GPSIQ_SC08, 12>;
    case 16: return w ? despread_rows<GPSIQ_SC16, 16> : despread_rows<GPSIQ_SC08, 16>;
    default: return nullptr;
    }
}
}  // namespace gpsiq
