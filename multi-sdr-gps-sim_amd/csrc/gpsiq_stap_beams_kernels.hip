// gpsiq_stap_beams_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_stap_beams (include/gpsiq_rows.h, "Space-time array"): up to
// eight tapped beams  y_b(n) = sum over e, t of w_b[e][t] x_e(n - t)  of the same element streams in one pass.
//   stap_beams_generic<IN, OUT>      every legal shape, and the cross-check: stap_combine's scheme with a loop over the beams around it
//   stap_beams_mfma<IN, OUT, TP>     the weights of all beams as operand A of v_mfma_i32_16x16x64_i8 in two digit planes, kept in
//                                    registers for the whole launch; the snapshots of 16 samples as operand B, taken from the element
//                                    streams as they lie in memory (gpsiq_stap_beams_geometry.h has the k-byte order, the tile and the
//                                    plane bounds); int16 input as two byte planes; the finish, the clamp and the counts in registers
// Pointers arrive by value as kernel arguments and are wave-uniform.  Every offset into a stream is 64 bits wide.  Sample n of a
// source is read only for 0 <= n < nsamp, sample m of a head only for 0 <= m < ntaps - 1, a destination is written for 0 <= n < nsamp
// and nowhere else, and only those of the beams < nbeams.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_stap_beams_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::load_pair;
using stream::sample_at;

typedef uint32_t beams_u32x4 __attribute__((ext_vector_type(4)));

// entry e of eight pointers: a chain of selects over the argument registers, so that a lane-dependent e needs no table in memory
__device__ __forceinline__ const uint8_t *beams_pointer_of(const uint8_t *const (&p)[kStapMaxElem], int e)
{
    const uint8_t *r = p[0];
#pragma unroll
    for (int k = 1; k < kStapMaxElem; ++k) r = e == k ? p[k] : r;
    return r;
}

// S finished samples of one beam, packed as they lie in its stream (16 bytes), to that stream from sample n0 on, those of them below
// nsamp: 16 bytes at once where the slot is whole and its address allows, four dwords where only the address does not (a destination
// is 4-byte aligned and a slot a multiple of 8 bytes into it), sample by sample at the span's end
template <int OUT, int S>
__device__ __forceinline__ void store_slot(uint8_t *dst, int64_t n0, int nsamp, const uint32_t (&v)[4])
{
    uint8_t *p = dst + (uint64_t) n0 * (2 * OUT);
    if (n0 + S <= (int64_t) nsamp) {
        if (!((uintptr_t) p & 15)) *reinterpret_cast<beams_u32x4 *>(p) = beams_u32x4{v[0], v[1], v[2], v[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j) reinterpret_cast<uint32_t *>(p)[j] = v[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (n0 + j < (int64_t) nsamp) {
                if (OUT == GPSIQ_SC16) reinterpret_cast<uint32_t *>(p)[j] = v[j];
                else reinterpret_cast<uint16_t *>(p)[j] = (uint16_t) (v[j >> 1] >> (16 * (j & 1)));
            }
    }
}

// sample j of a slot into its packed words (zeroed by the caller)
template <int OUT>
__device__ __forceinline__ void pack_sample(uint32_t (&v)[4], int j, int i, int q)
{
    if (OUT == GPSIQ_SC16) v[j] = ((uint32_t) i & 0xffffu) | ((uint32_t) q << 16);
    else v[j >> 1] |= (((uint32_t) i & 0xffu) | (((uint32_t) q & 0xffu) << 8)) << (16 * (j & 1));
}

// stream::finish in 32 bits for the matrix kernel, whose VALU it bounds: floor((acc + 2^(shift-1)) / 2^shift) is (acc >> shift) plus
// bit shift - 1 of acc (acc = q 2^shift + r with 0 <= r < 2^shift in two's complement, and r >= 2^(shift-1) is that bit), so the sum
// acc + 2^(shift-1), which can pass 2^31, is never formed.  down = shift - 1 (0 at shift 0), bit = 1 (0 at shift 0).
template <int OUT>
__device__ __forceinline__ int finish32(int acc, int shift, int down, int bit, unsigned &clipped)
{
    constexpr int QMAX = OUT == GPSIQ_SC08 ? 127 : 32767;
    const int y = (acc >> shift) + ((acc >> down) & bit);
    const int c = y < -QMAX ? -QMAX : y > QMAX ? QMAX : y;
    clipped += c != y;
    return c;
}

// the counts of a workgroup, one per beam, from its waves' partial counts: one atomic per beam that clamped anything
__device__ __forceinline__ void count_beams(const unsigned long long (&part)[kBeamsWaves][kBeamsMax], int nbeams, unsigned long long *count)
{
    __syncthreads();
    if ((int) threadIdx.x < nbeams) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < kBeamsWaves; ++w) sum += part[w][threadIdx.x];
        if (sum) atomicAdd(count + threadIdx.x, sum);
    }
}

// Arguments: the streams and heads, the coefficients (the weights from dword kBeamsWeightsAt on, [kBeamsMax][kStapMaxRows], re in the
// low half of a word, im in the high half), elements, taps, beams, the samples, shift, the destinations, the runs of the span
// (gpsiq_stap_beams_plan.h: kBeamsThreads slots each), the counters (zeroed by the host).  Slot u holds samples u S .. u S + S - 1,
// those of them below nsamp; thread t of run r takes slot kBeamsThreads r + t, once per beam.  A lane keeps a window of an element,
// the S + 7 samples that end with the slot's last, in registers: place j is sample n0 - 7 + j, and the places below 8 - ntaps are not
// read.  |acc| <= 65535 * 32768 < 2^31 by the host's bound on every beam's weights.
template <int IN, int OUT>
__global__ __launch_bounds__(kBeamsThreads) void stap_beams_generic(const StapSources src, const uint32_t *__restrict__ coef, int nelem, int ntaps,
                                                                    int nbeams, int nsamp, int shift, const BeamsDst dst, uint64_t runs,
                                                                    unsigned long long *__restrict__ count)
{
    constexpr int S = beams_lane_samples(OUT), H = kStapMaxTaps - 1, W = S + H;
    __shared__ unsigned long long part[kBeamsWaves][kBeamsMax];
    const int first = H - (ntaps - 1);
    for (int b = 0; b < nbeams; ++b) {
        const uint32_t *wt = coef + kBeamsWeightsAt + b * kStapMaxRows;
        uint8_t *out = dst.p[b];
        unsigned clipped = 0;
        for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
            const int64_t n0 = (int64_t) ((r * kBeamsThreads + threadIdx.x) * S);
            if (n0 >= (int64_t) nsamp) continue;
            const bool inside = n0 + S <= (int64_t) nsamp && n0 >= (int64_t) (ntaps - 1);      // every sample the slot reads is in the span
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
                    const uint32_t w = wt[e * ntaps + t];
                    const int re = (int) (int16_t) (w & 0xffffu), im = (int32_t) w >> 16;
#pragma unroll
                    for (int i = 0; i < S; ++i) {
                        ai[i] += re * xi[H + i - t] - im * xq[H + i - t];
                        aq[i] += re * xq[H + i - t] + im * xi[H + i - t];
                    }
                }
            }
            uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < S; ++i) {
                unsigned c = 0;                                        // (a place past the span still sums its neighbours: not an output)
                const int oi = stream::finish<OUT>(ai[i], shift, c), oq = stream::finish<OUT>(aq[i], shift, c);
                pack_sample<OUT>(v, i, oi, oq);
                if (n0 + i < (int64_t) nsamp) clipped += c;
            }
            store_slot<OUT, S>(out, n0, nsamp, v);
        }
        unsigned long long sum = clipped;
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][b] = sum;
    }
    count_beams(part, nbeams, count);
}

// an int8 sample pair as sample_at has it (I and Q sign-extended into the halves of a dword) back as its two stream bytes
__device__ __forceinline__ uint32_t pair_bytes(uint32_t v) { return (v & 0xffu) | ((v >> 8) & 0xff00u); }

// Arguments as stap_beams_generic's; of the coefficients the two digit planes of A in fragment order (lane l's 16 bytes at 16 l, plane
// d1 kBeamsPlaneBytes behind plane d0) and, for int16 input, the 16 row constants from dword kBeamsConstAt on.  The runs are chunks of
// 4 x 16 S samples; workgroup b takes the chunks b, b + gridDim.x, ...
// Staging.  Per chunk and element the samples c0 - H .. c0 + chunk - 1 and one dword more (gpsiq_stap_beams_geometry.h) go into LDS as the stream's own
// bytes -- int8: an aligned dword of the stream where both its samples are in the span, x(m) of the contract else; int16: the two byte
// planes lo' = (x & 255) - 128 and hi = x >> 8, so that a zero of the contract is (-128, 0) -- and that is the only place where the
// span's edges and the heads are told apart.
// Operand B.  Wave w takes samples 16 S w .. 16 S w + 16 S - 1 of the chunk in S steps; column col of step j is sample S col + j, so that
// a lane ends with S consecutive samples.  Lane (col, g) feeds k-bytes 16 g .. 16 g + 15: the windows of elements (8 / TP) g .. of that
// sample, 2 TP bytes each from sample n - TP + 1 on.  The S windows of an element overlap: the lane loads the S / 2 + TP / 2 + 1 dwords
// from the row's dword S col / 2 of the tile on once (an even sample), and window j starts j + 1 samples into them (j at TP = 1): at an
// odd sample it comes out by a 16-bit funnel shift.  Which steps are odd is the same for every lane and known when the loop is unrolled.
// Output.  D(row, col) is register row & 3 of lane col + 16 (row >> 2): lane (col, g) holds accI, accQ of beam 2 g and of beam 2 g + 1.
template <int IN, int OUT, int TP>
__global__ __launch_bounds__(kBeamsThreads) void stap_beams_mfma(const StapSources src, const uint32_t *__restrict__ coef, int nelem, int ntaps,
                                                                 int nbeams, int nsamp, int shift, const BeamsDst dst, uint64_t runs,
                                                                 unsigned long long *__restrict__ count)
{
    constexpr int S = beams_lane_samples(OUT), TILE = beams_tile_samples(OUT), CHUNK = beams_chunk_samples(OUT), BACK = beams_stage_back(TP);
    constexpr int RD = beams_row_dwords(OUT, TP), ME = beams_max_elem(TP), PL = IN == GPSIQ_SC16 ? 2 : 1;
    constexpr int P = 8 / TP, WD = beams_lane_dwords(OUT, TP), LEAD = TP > 1 ? 1 : 0;
    __shared__ uint32_t rows[PL][ME][RD];
    __shared__ unsigned long long part[kBeamsWaves][kBeamsMax];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
    const i32x4 a0 = reinterpret_cast<const i32x4 *>(coef)[lane];
    const i32x4 a1 = reinterpret_cast<const i32x4 *>(coef)[kBeamsPlaneBytes / 16 + lane];
    i32x4 rc = {0, 0, 0, 0};
    if (IN == GPSIQ_SC16) rc = reinterpret_cast<const i32x4 *>(coef + kBeamsConstAt)[g];
    uint8_t *const out0 = g == 0 ? dst.p[0] : g == 1 ? dst.p[2] : g == 2 ? dst.p[4] : dst.p[6];
    uint8_t *const out1 = g == 0 ? dst.p[1] : g == 1 ? dst.p[3] : g == 2 ? dst.p[5] : dst.p[7];
    const bool live0 = 2 * g < nbeams, live1 = 2 * g + 1 < nbeams;
    unsigned clip0 = 0, clip1 = 0;
    const int down = shift ? shift - 1 : 0, bit = shift ? 1 : 0;
    for (uint64_t r = blockIdx.x; r < runs; r += gridDim.x) {
        const int64_t c0 = (int64_t) r * CHUNK;
        __syncthreads();                                               // the chunk before has been read
        for (int i = tid; i < nelem * RD; i += kBeamsThreads) {
            const int e = i / RD, d = i - e * RD;
            const int64_t m = c0 - BACK + 2 * d;
            const uint8_t *p = beams_pointer_of(src.p, e), *hd = beams_pointer_of(src.head, e);
            const bool both = m >= 0 && m + 1 < (int64_t) nsamp;
            if (IN == GPSIQ_SC08) {
                uint32_t v;
                if (both) v = *reinterpret_cast<const uint32_t *>(p + (uint64_t) m * 2);
                else v = pair_bytes(sample_at<IN>(p, hd, m, nsamp, ntaps)) | (pair_bytes(sample_at<IN>(p, hd, m + 1, nsamp, ntaps)) << 16);
                rows[0][e][d] = v;
            } else {
                const uint32_t v0 = both ? load_pair<IN>(p, m) : sample_at<IN>(p, hd, m, nsamp, ntaps);
                const uint32_t v1 = both ? load_pair<IN>(p, m + 1) : sample_at<IN>(p, hd, m + 1, nsamp, ntaps);
                rows[0][e][d] = (pair_bytes(v0) | (pair_bytes(v1) << 16)) ^ 0x80808080u;                          // (x & 255) - 128 as a byte
                rows[PL - 1][e][d] = ((v0 >> 8) & 0xffu) | ((v0 >> 16) & 0xff00u) | (((v1 >> 8) & 0xffu) << 16) | (((v1 >> 16) & 0xff00u) << 16);   // x >> 8
            }
        }
        __syncthreads();
        if (c0 + wave * TILE >= (int64_t) nsamp) continue;             // (the same for every lane of the wave) nothing of the tile is in the span
        const int t0 = wave * TILE + S * col;                          // the lane's first sample of the chunk
        uint32_t win[PL][P][WD];
#pragma unroll
        for (int pl = 0; pl < PL; ++pl)
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int e = g * P + p;
#pragma unroll
                for (int i = 0; i < WD; ++i) win[pl][p][i] = 0u;
                if (e < nelem) {
#pragma unroll
                    for (int i = 0; i < WD; ++i) win[pl][p][i] = rows[pl][e][t0 / 2 + i];
                }
            }
        uint32_t v0[4] = {0u, 0u, 0u, 0u}, v1[4] = {0u, 0u, 0u, 0u};
        const int64_t n0 = c0 + t0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            i32x4 b[PL];
            const int at = (j + LEAD) >> 1;
            const bool odd = (j + LEAD) & 1;
#pragma unroll
            for (int pl = 0; pl < PL; ++pl) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    if (TP == 1) {
                        w[p >> 1] |= ((win[pl][p][at] >> (odd ? 16 : 0)) & 0xffffu) << (16 * (p & 1));
                    } else {
#pragma unroll
                        for (int k = 0; k < TP / 2; ++k)
                            w[p * (TP / 2) + k] = odd ? (win[pl][p][at + k] >> 16) | (win[pl][p][at + k + 1] << 16) : win[pl][p][at + k];
                    }
                }
                b[pl] = i32x4{(int) w[0], (int) w[1], (int) w[2], (int) w[3]};
            }
            const i32x4 zero = {0, 0, 0, 0};
            uint32_t acc[4];
            if (IN == GPSIQ_SC08) {
                const i32x4 p0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b[0], zero, 0, 0, 0);
                const i32x4 p1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b[0], zero, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = (uint32_t) p0[k] + ((uint32_t) p1[k] << 8);
            } else {
                const i32x4 p00 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b[0], zero, 0, 0, 0);
                i32x4 pmid = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b[PL - 1], zero, 0, 0, 0);
                pmid = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b[0], pmid, 0, 0, 0);
                const i32x4 p11 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b[PL - 1], zero, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = (uint32_t) p00[k] + ((uint32_t) pmid[k] << 8) + ((uint32_t) p11[k] << 16) + (uint32_t) rc[k];
            }
            unsigned c0i = 0, c1i = 0;                                 // (a column past the span still sums its neighbours: not an output)
            const int i0 = finish32<OUT>((int) acc[0], shift, down, bit, c0i), q0 = finish32<OUT>((int) acc[1], shift, down, bit, c0i);
            const int i1 = finish32<OUT>((int) acc[2], shift, down, bit, c1i), q1 = finish32<OUT>((int) acc[3], shift, down, bit, c1i);
            pack_sample<OUT>(v0, j, i0, q0);
            pack_sample<OUT>(v1, j, i1, q1);
            if (n0 + j < (int64_t) nsamp) { clip0 += c0i; clip1 += c1i; }
        }
        if (live0) store_slot<OUT, S>(out0, n0, nsamp, v0);
        if (live1) store_slot<OUT, S>(out1, n0, nsamp, v1);
    }
    // per wave in registers: the 16 lanes of a row group hold the counts of its two beams
    unsigned long long s0 = clip0, s1 = clip1;
    for (int off = 8; off >= 1; off >>= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
    if (col == 0) { part[wave][2 * g] = s0; part[wave][2 * g + 1] = s1; }
    count_beams(part, nbeams, count);
}

template <int IN, int OUT>
BeamsFn mfma_by_taps(int tp)
{
    return tp == 1 ? stap_beams_mfma<IN, OUT, 1> : tp == 2 ? stap_beams_mfma<IN, OUT, 2> : tp == 4 ? stap_beams_mfma<IN, OUT, 4> :
           tp == 8 ? stap_beams_mfma<IN, OUT, 8> : nullptr;
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_stap_beams.cpp looks up.  nullptr: no such kernel.
BeamsFn stap_beams_generic_kernel(int in_fmt, int out_fmt)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? stap_beams_generic<GPSIQ_SC08, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? stap_beams_generic<GPSIQ_SC08, GPSIQ_SC16> : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? stap_beams_generic<GPSIQ_SC16, GPSIQ_SC08> : out_fmt == GPSIQ_SC16 ? stap_beams_generic<GPSIQ_SC16, GPSIQ_SC16> : nullptr;
    return nullptr;
}

BeamsFn stap_beams_mfma_kernel(int in_fmt, int out_fmt, int padded_taps)
{
    if (in_fmt == GPSIQ_SC08) return out_fmt == GPSIQ_SC08 ? mfma_by_taps<GPSIQ_SC08, GPSIQ_SC08>(padded_taps) : out_fmt == GPSIQ_SC16 ? mfma_by_taps<GPSIQ_SC08, GPSIQ_SC16>(padded_taps) : nullptr;
    if (in_fmt == GPSIQ_SC16) return out_fmt == GPSIQ_SC08 ? mfma_by_taps<GPSIQ_SC16, GPSIQ_SC08>(padded_taps) : out_fmt == GPSIQ_SC16 ? mfma_by_taps<GPSIQ_SC16, GPSIQ_SC16>(padded_taps) : nullptr;
    return nullptr;
}
}  // namespace gpsiq
