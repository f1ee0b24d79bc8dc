// gpsiq_acquire_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_acquire (include/gpsiq_rows.h, "Acquisition"): a blind
// search of one span of a stream for a list of satellites over Doppler bins and sample shifts.  Everything up to the power is integer
// arithmetic, so the correlations are a pure function of (arguments, stream bytes); the power is taken with __dmul_rn / __dadd_rn in
// the order the contract states, dwell by dwell.
//   acquire_generic   the contract written straight down on the VALU: a lane owns a shift, wipes every sample itself and sums in 64
//                     bits.  The cross-check, and the fallback for shapes the planner refuses the matrix path.
//   acquire_wipe      stage one of the matrix path: the carrier once per (bin, sample); the wiped yi, yq leave as planes of balanced
//                     base-256 digits (3 for int8, 4 for int16), laid out so that a wave's A fragment of a k-step is 1 KiB in a row.
//   acquire_mfma      stage two: v_mfma_i32_16x16x64_i8 of 16 digit rows x 64 samples against 64 samples x 16 shifts of the +-1 code
//                     (a banded Toeplitz operand), the digits recombined in int64, the power taken per dwell in ascending order.
//   acquire_peaks     the maximum over the shifts of every (satellite, bin), lowest shift on a tie.
// The Toeplitz operand: a tile's 16 columns are shifts 16 apart, so the 16 code bytes a lane needs start at a multiple of 16 of ONE
// copy of the sampled code, shifted by the residue of (shift + dwell offset) mod 16; the 16 zero-padded copies live in LDS and every
// B fragment is one aligned ds_read_b128.  A wave owns 256 consecutive shifts -- 16 tiles, one per residue -- of one row tile, and
// multiplies each plane fragment it loads by all 16 code fragments.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_acquire_geometry.h"
#include "gpsiq_signal.h"
#include "gpsiq_stream.h"

namespace gpsiq {
namespace {

using stream::i32x4;

// +1 / -1 of replica sample n: chip ((n * code_step) >> 56) % 1023 of the satellite whose packed code is ext (bit set: -1)
__device__ __forceinline__ int acq_code(const uint32_t *ext, uint64_t code_step, uint32_t n)
{
    const unsigned __int128 t = (unsigned __int128) code_step * (unsigned __int128) n;
    const uint32_t chip = (uint32_t) ((uint64_t) (t >> GPSIQ_CODE_FRAC_BITS) % GPSIQ_CA_SEQ_LEN);
    return ((ext[chip >> 5] >> (chip & 31)) & 1u) ? -1 : 1;
}

}  // namespace

// ---------------------------------------------------------------------------
// Generic kernel.  Thread = (satellite, bin, shift); dwell by dwell it walks the ncoh samples, the carrier phase by one 64-bit add per
// sample (the product m * step wraps mod 2^64, a multiple of 2^59), the code phase as a chip
// counter and a 56-bit fraction that every lane steps alike.
template <int FMT>
__global__ __launch_bounds__(kAcqThreads) void acquire_generic(
    const uint8_t *__restrict__ src, const DeviceTables *__restrict__ tab, const uint8_t *__restrict__ prns, int nshift, int ncoh, int nnoncoh,
    int hop, int ndopp, uint64_t code_step, uint64_t carr_step0, uint64_t carr_step_inc, double *__restrict__ power,
    gpsiq_despread_sum_t *__restrict__ corr)
{
    __shared__ uint32_t unit[512];
    __shared__ uint32_t ext[kPrnExtWords];
    const int p = blockIdx.z, d = blockIdx.y;
    stage_unit<kAcqThreads>(tab, unit);
    if (threadIdx.x < kPrnExtWords) ext[threadIdx.x] = tab->prn_ext[prns[p] - 1][threadIdx.x];
    __syncthreads();
    const uint64_t s = (uint64_t) blockIdx.x * kAcqThreads + threadIdx.x;
    if (s >= (uint64_t) nshift) return;
    const uint64_t step = carr_step0 + (uint64_t) d * carr_step_inc;
    const uint64_t cell = ((uint64_t) p * (uint64_t) ndopp + (uint64_t) d) * (uint64_t) nshift + s;
    double acc = 0.0;
    for (int k = 0; k < nnoncoh; ++k) {
        const uint64_t m0 = s + (uint64_t) k * (uint64_t) hop;
        uint64_t P = m0 * step;
        int64_t xi = 0, xq = 0;
        uint64_t frac = 0;                                         // n * code_step, as chip (mod 1023) and 56-bit fraction
        uint32_t chip = 0;
        for (int n = 0; n < ncoh; ++n) {
            int si, sq;
            load_iq<FMT>(src, m0 + (uint64_t) n, &si, &sq);           // (every sample a shift reads lies inside the stream)
            const uint32_t v = unit[(uint32_t) ((P & kCarrFracMask) >> (GPSIQ_CARR_FRAC_BITS - 9))];
            const int rc = (int16_t) (v & 0xffffu), rs = (int32_t) v >> 16;
            const bool neg = (ext[chip >> 5] >> (chip & 31)) & 1u;
            const int yi = si * rc + sq * rs, yq = sq * rc - si * rs;      // each product below 2^24
            xi += (int64_t) (neg ? -yi : yi);
            xq += (int64_t) (neg ? -yq : yq);
            P += step;
            frac += code_step & kCodeFracMask;
            chip += (uint32_t) (code_step >> GPSIQ_CODE_FRAC_BITS) + (uint32_t) (frac >> GPSIQ_CODE_FRAC_BITS);      // at most 256 chips on
            frac &= kCodeFracMask;
            if (chip >= GPSIQ_CA_SEQ_LEN) chip -= GPSIQ_CA_SEQ_LEN;
        }
        if (corr) {
            gpsiq_despread_sum_t *o = corr + ((uint64_t) p * (uint64_t) ndopp + (uint64_t) d) * (uint64_t) nnoncoh * (uint64_t) nshift + (uint64_t) k * (uint64_t) nshift + s;
            o->i = xi; o->q = xq;
        }
        const double fi = (double) xi, fq = (double) xq;          // exact: |X| < 2^44
        acc = __dadd_rn(acc, __dadd_rn(__dmul_rn(fi, fi), __dmul_rn(fq, fq)));
    }
    power[cell] = acc;
}

// ---------------------------------------------------------------------------
// Stage one.  Thread = (row tile, bin of the tile, four consecutive samples).  A tile is 16 rows: row 4 * (2 * bin_of_tile + iq) + digit,
// so that the four output registers of a lane of the 16x16 product are the four digits of one (bin, I or Q).  Memory order inside a
// tile: [sample / 16][row][sample % 16] -- the 16 rows x 64 samples of a k-step are 1 KiB in a row, lane l's fragment at 16 l.
// Samples at or past `span` (the plane's tail), the fourth digit row of int8 and the second bin of an odd last tile are written as
// zeros: the matrix stage reads every byte of its planes.
// Balanced digits: y = sum d_i 256^i with d_i in [-128, 127]; |y| <= 128 * 355 needs three (three hold [-8 421 504, 8 355 711]),
// |y| <= 32768 * 355 = 11 632 640 needs four.
template <int FMT>
__global__ __launch_bounds__(kAcqThreads) void acquire_wipe(
    const uint8_t *__restrict__ src, const DeviceTables *__restrict__ tab, uint64_t span, uint64_t npad, int ndopp, int row_tiles,
    uint64_t carr_step0, uint64_t carr_step_inc, uint8_t *__restrict__ planes)
{
    constexpr int ND = FMT == GPSIQ_SC16 ? 4 : 3;
    __shared__ uint32_t unit[512];
    stage_unit<kAcqThreads>(tab, unit);
    __syncthreads();
    const uint64_t quads = npad / 4;
    const uint64_t t = (uint64_t) blockIdx.x * kAcqThreads + threadIdx.x;
    if (t >= (uint64_t) row_tiles * kAcqBinsPerTile * quads) return;
    const uint64_t slot = t / quads, m4 = (t % quads) * 4;
    const int tile = (int) (slot / kAcqBinsPerTile), bl = (int) (slot % kAcqBinsPerTile), d = tile * kAcqBinsPerTile + bl;
    uint32_t w[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};                // [iq][digit]: four samples' digits, one byte each
    if (d < ndopp) {
        const uint64_t step = carr_step0 + (uint64_t) d * carr_step_inc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t m = m4 + (uint64_t) j;
            if (m >= span) break;
            int si, sq;
            load_iq<FMT>(src, m, &si, &sq);
            const uint32_t v = unit[(uint32_t) (((m * step) & kCarrFracMask) >> (GPSIQ_CARR_FRAC_BITS - 9))];
            const int rc = (int16_t) (v & 0xffffu), rs = (int32_t) v >> 16;
            int y[2] = {si * rc + sq * rs, sq * rc - si * rs};
#pragma unroll
            for (int iq = 0; iq < 2; ++iq) {
#pragma unroll
                for (int g = 0; g < ND; ++g) {
                    const int dg = ((y[iq] + 128) & 255) - 128;
                    w[iq][g] |= ((uint32_t) dg & 0xffu) << (8 * j);
                    y[iq] = (y[iq] - dg) >> 8;                     // exact: the difference is a multiple of 256
                }
            }
        }
    }
    uint8_t *base = planes + (uint64_t) tile * kAcqTileRows * npad + (m4 >> 4) * (kAcqTileRows * 16) + (m4 & 15);
#pragma unroll
    for (int iq = 0; iq < 2; ++iq)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<uint32_t *>(base + (4 * (2 * bl + iq) + g) * 16) = w[iq][g];
}

// ---------------------------------------------------------------------------
// Stage two.  Workgroup = (block of 256 shifts S0 .. S0 + 255, four row tiles, satellite); wave w owns row tile 4 * blockIdx.y + w.
// Accumulator a (0..15) of a wave is the 16x16 tile of shifts S0 + 16 c + a, c the column.  For dwell k with offset h = k * hop, k-step t
// covers plane samples m0 .. m0 + 63, m0 = S0 + (h & ~15) + 64 t.  The MFMA sums over all 64 k positions and gives lane (c, g) bytes j of
// A and of B the same k, so any assignment serves as long as both operands use it: lane l = (i, g) takes plane bytes m0 + 16 g + j of
// row i, and lane (c, g) takes code bytes n = m0 + 16 g + j - (S0 + 16 c + a + h) = 16 u + j - rho with
//     w = a + (h & 15),  rho = w & 15,  u = 4 t + g - c - (w >> 4)
// i.e. bytes 16 u .. 16 u + 15 of copy rho, copy_rho[x] = ca[x - rho] (zero outside [0, ncoh)); u outside [0, ncoh / 16] is all zeros:
// every copy has a unit of 16 zeros in front and one behind, and u is clamped to [-1, ncoh / 16 + 1] (a compare, a select and a minimum per fragment), so no fragment
// needs a select.  A copy is ncoh + 48 bytes.
// After the last k-step lane (c, g) holds, per accumulator, the four digit sums of (bin 2 tile + (g >> 1), I or Q by g & 1): each at
// most 128 * ncoh < 2^31.  They are recombined in int64, the Q lane's value crosses to the I lane 16 lanes below, which takes the power.
template <int ND>
__global__ __launch_bounds__(kAcqWaves * 64) void acquire_mfma(
    const uint8_t *__restrict__ planes, const DeviceTables *__restrict__ tab, const uint8_t *__restrict__ prns, uint64_t npad, int row_tiles,
    int nshift, int ncoh, int nnoncoh, int hop, int ndopp, uint64_t code_step, int ksteps, double *__restrict__ power,
    gpsiq_despread_sum_t *__restrict__ corr)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t copies[];       // [16][16 zeros | ncoh + 16 | 16 zeros]
    __shared__ uint32_t ext[kPrnExtWords];
    const int tid = threadIdx.x, p = blockIdx.z;
    if (tid < kPrnExtWords) ext[tid] = tab->prn_ext[prns[p] - 1][tid];
    __syncthreads();
    const int clen = ncoh + kAcqCopyPad;
    for (int x = tid; x < clen; x += kAcqWaves * 64)                       // copy 0: sixteen zeros, the sampled code, zeros behind it
        copies[x] = x >= 16 && x < ncoh + 16 ? (uint8_t) (int8_t) acq_code(ext, code_step, (uint32_t) (x - 16)) : (uint8_t) 0;
    __syncthreads();
    for (int e = clen + tid; e < 16 * clen; e += kAcqWaves * 64) {         // copy rho: copy 0 moved up by rho, zeros below
        const int rho = e / clen, x = e - rho * clen;
        copies[e] = x >= rho ? copies[x - rho] : (uint8_t) 0;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int tile = (int) blockIdx.y * kAcqWaves + wave;
    if (tile >= row_tiles) return;                                         // the whole wave, behind the last barrier
    const int c = lane & 15, g = lane >> 4;
    const uint64_t S0 = (uint64_t) blockIdx.x * kAcqBlockShifts;
    const uint8_t *tile_planes = planes + (uint64_t) tile * kAcqTileRows * npad + (uint64_t) lane * 16;
    const int ulast = (ncoh >> 4) + 1;                                     // the zero unit behind a copy
    const int d = tile * kAcqBinsPerTile + (g >> 1);
    const bool owner = (g & 1) == 0 && d < ndopp;                          // the I lanes of bins that exist

    double acc[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) acc[a] = 0.0;

    for (int k = 0; k < nnoncoh; ++k) {
        const uint64_t h = (uint64_t) k * (uint64_t) hop;
        const int hr = (int) (h & 15);
        const uint8_t *a_ptr = tile_planes + (S0 + (h & ~UINT64_C(15))) * 16;
        i32x4 D[16];
#pragma unroll
        for (int a = 0; a < 16; ++a) D[a] = i32x4{0, 0, 0, 0};
        for (int t = 0; t < ksteps; ++t) {
            const i32x4 A = *reinterpret_cast<const i32x4 *>(a_ptr + (uint64_t) t * (kAcqK * 16));
            const int u0 = 4 * t + g - c;
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                const int w = a + hr, u = u0 - (w >> 4);
                const int unit = (u < -1 ? -1 : u > ulast ? ulast : u) + 1;       // 0 and ulast + 1: the zero units
                const i32x4 B = *reinterpret_cast<const i32x4 *>(copies + (w & 15) * clen + unit * 16);
                D[a] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, D[a], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            int64_t x = (int64_t) D[a][0] + ((int64_t) D[a][1] << 8) + ((int64_t) D[a][2] << 16);
            if (ND == 4) x += (int64_t) D[a][3] << 24;
            const int64_t xq = __shfl_down(x, 16, 64);                     // the Q lane of the same bin and column
            const uint64_t s = S0 + (uint64_t) (16 * c + a);
            if (owner && s < (uint64_t) nshift) {
                if (corr) {
                    gpsiq_despread_sum_t *o = corr + (((uint64_t) p * (uint64_t) ndopp + (uint64_t) d) * (uint64_t) nnoncoh + (uint64_t) k) * (uint64_t) nshift + s;
                    o->i = x; o->q = xq;
                }
                const double fi = (double) x, fq = (double) xq;
                acc[a] = __dadd_rn(acc[a], __dadd_rn(__dmul_rn(fi, fi), __dmul_rn(fq, fq)));
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 16; ++a) {
        const uint64_t s = S0 + (uint64_t) (16 * c + a);
        if (owner && s < (uint64_t) nshift) power[((uint64_t) p * (uint64_t) ndopp + (uint64_t) d) * (uint64_t) nshift + s] = acc[a];
    }
}

// ---------------------------------------------------------------------------
// One wave per (satellite, bin): the largest power over the shifts, lowest shift on a tie.  Powers are non-negative and never NaN
// (sums of squares of finite values below 2^89).
__global__ __launch_bounds__(kAcqThreads) void acquire_peaks(const double *__restrict__ power, uint64_t rows, int nshift, gpsiq_acquire_peak_t *__restrict__ peaks)
{
    const uint64_t row = (uint64_t) blockIdx.x * (kAcqThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const double *r = power + row * (uint64_t) nshift;
    double best = -1.0;
    int at = 0;
    for (int s = lane; s < nshift; s += 64) {
        const double v = r[s];
        if (v > best) { best = v; at = s; }                               // ascending s: the first of equals stays
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oa = __shfl_xor(at, off, 64);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) { peaks[row].power = best; peaks[row].shift = at; peaks[row].reserved = 0; }
}

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_acquire.cpp looks up with the values of a plan (gpsiq_acquire_plan.h).
AcquireGenericFn acquire_generic_kernel(int fmt)
{
    return fmt == GPSIQ_SC16 ? acquire_generic<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? acquire_generic<GPSIQ_SC08> : nullptr;
}
AcquireWipeFn acquire_wipe_kernel(int fmt)
{
    return fmt == GPSIQ_SC16 ? acquire_wipe<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? acquire_wipe<GPSIQ_SC08> : nullptr;
}
AcquireMfmaFn acquire_mfma_kernel(int digits)
{
    return digits == 4 ? acquire_mfma<4> : digits == 3 ? acquire_mfma<3> : nullptr;
}
AcquirePeaksFn acquire_peaks_kernel() { return acquire_peaks; }
}  // namespace gpsiq
