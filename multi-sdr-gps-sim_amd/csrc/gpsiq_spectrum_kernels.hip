// gpsiq_spectrum_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_spectrum (include/gpsiq_rows.h, "Spectrum"): the exact
// integer power spectrum of ONE contiguous span of interleaved I,Q samples, int8 or int16 -- a dense DFT over the 512-entry carrier
// table, the Hann window across bins, a flooring shift, and the squares summed per group of segments in uint64.
//   spectrum_generic<FMT>   both formats, every nfft / hop / window: a workgroup stages a segment in LDS, a thread accumulates whole
//                           bins (int32 partials of kSpecChunk terms into int64), Hann neighbours come through LDS
//   spectrum_mfma           int8 input: v_mfma_i32_16x16x64_i8 with the TABLE (window folded in) as operand A in two digit planes and
//                           the stream as operand B, a column a segment (gpsiq_spectrum_geometry.h has the tiles)
// Both end in the same cell(): shift each component, square, add.  The host has checked 2 navg Ys^2 <= 2^64 - 1 with Ys >= |Y'|
// (gpsiq_spectrum_plan.h: spectrum_fits), so a cell fits uint64 and so does every sum of up to navg of them, in any order.
// Every offset into src is 64 bits wide.  Sample m of the span is read only for m < (ngroups navg - 1) hop + nfft.  No workgroup
// waits for another: they meet in atomic adds into power, which the host has zeroed.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_spectrum_geometry.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;
using stream::load_pair;

// Yi'^2 + Yq'^2: the shift is arithmetic and floors; |Y'| <= Ys < 2^32 by the host's bound, so each square fits uint64 and so does their sum
__device__ __forceinline__ unsigned long long cell(long long yi, long long yq, int shift)
{
    yi >>= shift;
    yq >>= shift;
    const unsigned long long ai = (unsigned long long) (yi < 0 ? -yi : yi), aq = (unsigned long long) (yq < 0 ? -yq : yq);
    return ai * ai + aq * aq;
}

// Arguments: the span, the table as 512 dwords (cos in the low half, sin in the high half), nfft, hop, window, shift, navg, the units
// of a group, the units of the launch (gpsiq_spectrum_plan.h), power [ngroups][nfft] (zeroed by the host).
// blockDim.x = min(nfft, 256); thread t owns bins t and, at nfft 512, t + 256.
// Partial sums: |I c + Q s| <= 250 (|I| + |Q|) <= 250 * 65536, kSpecChunk = 32 of them are at most 524 288 000 < 2^31; a bin is at
// most 512 * 250 * 65536 < 2^34 and the windowed bin four times that, < 2^36: int64 throughout.
template <int FMT>
__global__ __launch_bounds__(kSpecThreads) void spectrum_generic(const uint8_t *__restrict__ src, const uint32_t *__restrict__ table, int nfft, int hop,
                                                                  int window, int shift, int navg, uint64_t per, uint64_t units,
                                                                  unsigned long long *__restrict__ power)
{
    __shared__ uint32_t win[kSpecMaxFft];
    __shared__ uint32_t tab[512];
    __shared__ long long xs[2][kSpecMaxFft];
    const int tid = threadIdx.x, nthr = blockDim.x, bins = nfft / nthr;
    for (int i = tid; i < 512; i += nthr) tab[i] = table[i];
    const int T = 512 / nfft;
    for (uint64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint64_t g = u / per, r = u % per;
        const uint64_t s0 = g * (uint64_t) navg + r * kSpecRun;
        const uint64_t left = (uint64_t) navg - r * kSpecRun, s1 = s0 + (left < (uint64_t) kSpecRun ? left : (uint64_t) kSpecRun);
        unsigned long long sum[2] = {0, 0};
        for (uint64_t s = s0; s < s1; ++s) {
            __syncthreads();                                               // the segment before has been read, its bins' neighbours too
            for (int i = tid; i < nfft; i += nthr) win[i] = load_pair<FMT>(src, (int64_t) (s * (uint64_t) hop + (uint64_t) i));
            __syncthreads();
            long long xi[2] = {0, 0}, xq[2] = {0, 0};
            for (int b = 0; b < bins; ++b) {
                const int k = tid + b * nthr;
                const int step = (k * T) & 511;
                int idx = 0;
                for (int n0 = 0; n0 < nfft; n0 += kSpecChunk) {
                    int pi = 0, pq = 0;
#pragma unroll 8
                    for (int j = 0; j < kSpecChunk; ++j) {
                        const uint32_t v = win[n0 + j], t = tab[idx];
                        const int I = (int) (int16_t) (v & 0xffffu), Q = (int32_t) v >> 16;
                        const int c = (int) (int16_t) (t & 0xffffu), sn = (int32_t) t >> 16;
                        pi += I * c + Q * sn;
                        pq += Q * c - I * sn;
                        idx = (idx + step) & 511;
                    }
                    xi[b] += pi;
                    xq[b] += pq;
                }
                if (window) { xs[0][k] = xi[b]; xs[1][k] = xq[b]; }
            }
            if (window) {
                __syncthreads();
                for (int b = 0; b < bins; ++b) {
                    const int k = tid + b * nthr, lo = (k - 1) & (nfft - 1), hi = (k + 1) & (nfft - 1);
                    xi[b] = 2 * xi[b] - xs[0][lo] - xs[0][hi];
                    xq[b] = 2 * xq[b] - xs[1][lo] - xs[1][hi];
                }
            }
            for (int b = 0; b < bins; ++b) sum[b] += cell(xi[b], xq[b], shift);
        }
        for (int b = 0; b < bins; ++b) atomicAdd(power + g * (uint64_t) nfft + (uint64_t) (tid + b * nthr), sum[b]);
    }
}

// Arguments: the span (int8), the two digit planes of A in fragment order, nfft, hop, shift, navg, the segments that are read
// (ngroups navg), the segments of a pass, the passes of the launch and of a workgroup (gpsiq_spectrum_plan.h), power.
// Dynamic LDS: [nfft] uint64 sums, [nfft] uint32 group tags (+ padding to 16 nfft bytes), then the window of the pass in padded
// chunks (gpsiq_spectrum_geometry.h), 16-byte aligned.
// Lanes (gpsiq_acquire_kernels.hip measured the map): A lane l feeds row l & 15 with bytes k = 16 (l >> 4) + j, B lane l feeds column
// l & 15 with the same k, D(row, col) is register row & 3 of lane col + 16 (row >> 2): lane (col, q) ends with i and q of bins
// 8 rt + 2 q and 8 rt + 2 q + 1 of segment col.
// Digit planes: an entry a of A (|a| <= 250 rectangular, <= 1000 Hann) is d0 + 256 d1 with d0 = ((a + 128) & 255) - 128 in
// [-128, 127] and |d1| <= 4.  Partial sums over the 2 nfft <= 1024 bytes of a segment, |x| <= 128: |P0| <= 128 * 128 * 1024 = 2^24,
// |P1| <= 4 * 128 * 1024 = 2^19, |256 P1| <= 2^27, and Y = P0 + 256 P1 is the contract's Y, |Y| <= 4 * 512 * 500 * 128 < 2^27: all
// inside int32.  Bytes of the window past the last segment that is read are staged as zeros; their columns are not added.
// Sums: the lane with col == 0 of (wave, q) owns bins 8 rt + 2 q, 8 rt + 2 q + 1 of the wave's row tiles rt = wave, wave + 4, ...; it
// alone reads and writes their LDS sums and tags.  A tile whose sixteen segments lie in one group is summed across its columns and
// added to the LDS sum of that group, which goes to power in one atomic when the bin meets another group and at the end; the columns
// of a tile that spans groups add their cells to power themselves.
__global__ __launch_bounds__(kSpecThreads) void spectrum_mfma(const uint8_t *__restrict__ src, const uint8_t *__restrict__ planes, int nfft, int hop, int shift,
                                                               int navg, uint32_t used, int cols, uint64_t passes, uint64_t per,
                                                               unsigned long long *__restrict__ power)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t spec_lds[];
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(spec_lds);
    uint32_t *tags = reinterpret_cast<uint32_t *>(spec_lds + 8 * nfft);
    uint8_t *win = spec_lds + spectrum_mfma_sums_bytes(nfft);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, q = lane >> 4;
    const int ksteps = spectrum_ksteps(nfft), row_tiles = spectrum_row_tiles(nfft);
    const int chunk_bytes = 2 * hop, stride = spectrum_chunk_stride(hop), chunk_dwords = hop / 2;
    const int window_dwords = (cols - 1 + nfft / hop) * chunk_dwords;
    const size_t plane_bytes = (size_t) spectrum_plane_bytes(nfft);
    const uint64_t limit_dw = ((uint64_t) (used - 1) * (uint64_t) hop + (uint64_t) nfft) / 2;       // dwords of the span that are read
    constexpr uint32_t kNoGroup = 0xffffffffu;                                                       // (groups are < 2^31)
    for (int k = tid; k < nfft; k += kSpecThreads) { sums[k] = 0; tags[k] = kNoGroup; }
    __syncthreads();
    const uint64_t p_begin = (uint64_t) blockIdx.x * per, p_end = p_begin + per < passes ? p_begin + per : passes;
    for (uint64_t pass = p_begin; pass < p_end; ++pass) {
        const uint64_t seg0 = pass * (uint64_t) cols;
        const uint64_t base_dw = seg0 * (uint64_t) chunk_dwords;
        __syncthreads();                                                   // the pass before has read its window
        for (int i = tid; i < window_dwords; i += kSpecThreads) {
            const int ch = i / chunk_dwords, w = i - ch * chunk_dwords;
            const uint64_t dw = base_dw + (uint64_t) i;
            const uint32_t v = dw < limit_dw ? reinterpret_cast<const uint32_t *>(src)[dw] : 0u;
            *reinterpret_cast<uint32_t *>(win + ch * stride + 4 * w) = v;
        }
        __syncthreads();
        const uint64_t here = (uint64_t) used - seg0;                      // segments from seg0 on (>= 1)
        const int nseg = here < (uint64_t) cols ? (int) here : cols;       // segments of this pass
        const int ntile = (nseg + kSpecTileCols - 1) / kSpecTileCols;
        for (int rt = wave; rt < row_tiles; rt += kSpecThreads / 64) {
            i32x4 d0[kSpecMaxColTiles], d1[kSpecMaxColTiles];
#pragma unroll
            for (int c = 0; c < kSpecMaxColTiles; ++c) { d0[c] = i32x4{0, 0, 0, 0}; d1[c] = i32x4{0, 0, 0, 0}; }
            const uint8_t *a_ptr = planes + (size_t) rt * (size_t) ksteps * (kSpecK * 16) + (size_t) lane * 16;
            for (int t = 0; t < ksteps; ++t) {
                const i32x4 a0 = *reinterpret_cast<const i32x4 *>(a_ptr + (size_t) t * (kSpecK * 16));
                const i32x4 a1 = *reinterpret_cast<const i32x4 *>(a_ptr + plane_bytes + (size_t) t * (kSpecK * 16));
                const int ch = (kSpecK * t) / chunk_bytes;
                const uint8_t *b_ptr = win + (col + ch) * stride + (kSpecK * t - ch * chunk_bytes) + 16 * q;
#pragma unroll
                for (int c = 0; c < kSpecMaxColTiles; ++c) {
                    if (c < ntile) {
                        const i32x4 b = *reinterpret_cast<const i32x4 *>(b_ptr + c * kSpecTileCols * stride);
                        d0[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, d0[c], 0, 0, 0);
                        d1[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, d1[c], 0, 0, 0);
                    }
                }
            }
            const int k0 = kSpecTileBins * rt + 2 * q;                     // this lane's bins: k0, k0 + 1
#pragma unroll
            for (int c = 0; c < kSpecMaxColTiles; ++c) {
                if (c >= ntile) break;
                const int first = c * kSpecTileCols, last = first + kSpecTileCols - 1 < nseg - 1 ? first + kSpecTileCols - 1 : nseg - 1;
                const bool valid = first + col <= last;
                const uint32_t g_first = (uint32_t) ((seg0 + (uint64_t) first) / (uint64_t) navg), g_last = (uint32_t) ((seg0 + (uint64_t) last) / (uint64_t) navg);
                unsigned long long c0 = cell(d0[c][0] + 256 * d1[c][0], d0[c][1] + 256 * d1[c][1], shift);
                unsigned long long c1 = cell(d0[c][2] + 256 * d1[c][2], d0[c][3] + 256 * d1[c][3], shift);
                if (!valid) { c0 = 0; c1 = 0; }
                if (g_first == g_last) {                                   // (the same for every lane of the wave)
#pragma unroll
                    for (int off = 8; off >= 1; off >>= 1) { c0 += __shfl_xor(c0, off, 64); c1 += __shfl_xor(c1, off, 64); }
                    if (col == 0) {
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            const int k = k0 + b;
                            if (tags[k] != g_first) {
                                if (tags[k] != kNoGroup) atomicAdd(power + (uint64_t) tags[k] * (uint64_t) nfft + (uint64_t) k, sums[k]);
                                tags[k] = g_first;
                                sums[k] = 0;
                            }
                            sums[k] += b ? c1 : c0;
                        }
                    }
                } else if (valid) {
                    const uint64_t g = (seg0 + (uint64_t) (first + col)) / (uint64_t) navg;
                    atomicAdd(power + g * (uint64_t) nfft + (uint64_t) k0, c0);
                    atomicAdd(power + g * (uint64_t) nfft + (uint64_t) (k0 + 1), c1);
                }
            }
        }
    }
    if (col == 0)
        for (int rt = wave; rt < row_tiles; rt += kSpecThreads / 64)
            for (int b = 0; b < 2; ++b) {
                const int k = kSpecTileBins * rt + 2 * q + b;
                if (tags[k] != kNoGroup) atomicAdd(power + (uint64_t) tags[k] * (uint64_t) nfft + (uint64_t) k, sums[k]);
            }
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_spectrum.cpp looks up.  nullptr: no such kernel.
SpectrumGenericFn spectrum_generic_kernel(int fmt)
{
    return fmt == GPSIQ_SC08 ? spectrum_generic<GPSIQ_SC08> : fmt == GPSIQ_SC16 ? spectrum_generic<GPSIQ_SC16> : nullptr;
}

SpectrumMfmaFn spectrum_mfma_kernel(int fmt) { return fmt == GPSIQ_SC08 ? spectrum_mfma : nullptr; }
}  // namespace gpsiq
