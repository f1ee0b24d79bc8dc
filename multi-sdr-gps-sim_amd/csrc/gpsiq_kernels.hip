// gpsiq_kernels.hip — gfx950 (MI355X, wave64) kernels of libgpsiq.
//
// Replaces the per-sample loop of Mictronics/multi-sdr-gps-sim gps.c:2767-2836 and
// the pack of gps.c:2839-2846 with the closed-form integer NCO model of
// include/gpsiq.h.  One workgroup synthesises one tile of one 0.1 s block:
//   * the per-channel gain LUT  TC/TS[k] = (int)(table[k]*gain)  (gps.c:2781-2782
//     with dataBit*codeCA factored out) is built once per workgroup into LDS,
//     packed (I | Q<<16) as two int16 — sums are taken mod 2^16, which is exactly
//     what the reference's (short) store keeps (gps.c:2834-2835);
//   * the 1023-chip C/A codes are staged in LDS bit-packed, with a wrap-around tail;
//   * nothing is read from HBM per sample: the only traffic is the IQ write.
// No MFMA: there is no contraction in this path; it is integer VALU + LDS gather.
#include <hip/hip_runtime.h>

#include <array>

#include "gpsiq_ctx.h"
#include "gpsiq_geometry.h"
#include "gpsiq_noise.h"
#include "gpsiq_signal.h"

namespace gpsiq {

constexpr int kMaxChan = GPSIQ_MAX_CHAN;

typedef short s16x2 __attribute__((ext_vector_type(2)));

// Workgroup prologue shared by both kernels: descriptors, gain LUTs and C/A codes to LDS.
template <int NT>
__device__ __forceinline__ void stage_block(const gpsiq_qchan_t *__restrict__ q, int nchan,
                                            const DeviceTables *__restrict__ tab,
                                            gpsiq_qchan_t *qs, uint32_t (*lut)[512],
                                            uint32_t (*ext)[kPrnExtWords])
{
    const int tid = threadIdx.x;
    // 48-byte descriptors as 12 dwords each
    for (int i = tid; i < nchan * 12; i += NT)
        reinterpret_cast<uint32_t *>(qs)[i] = reinterpret_cast<const uint32_t *>(q)[i];
    __syncthreads();
    for (int e = tid; e < nchan * 512; e += NT) {
        const int c = e >> 9, k = e & 511;
        if (qs[c].prn == 0) continue;
        const double g = qs[c].gain;
        // (int)(int * double): exact int->double, one IEEE multiply, truncation toward 0
        const int ts = (int) ((double) dev_sin512(tab->quarter_wave, k) * g);
        const int tc = (int) ((double) dev_sin512(tab->quarter_wave, k + 128) * g);
        lut[c][k] = ((uint32_t) tc & 0xffffu) | ((uint32_t) ts << 16);
    }
    for (int e = tid; e < nchan * kPrnExtWords; e += NT) {
        const int c = e / kPrnExtWords, w = e % kPrnExtWords;
        if (qs[c].prn == 0) continue;
        ext[c][w] = tab->prn_ext[qs[c].prn - 1][w];
    }
    __syncthreads();
}

template <int FMT>
__device__ __forceinline__ void store_sample(uint8_t *__restrict__ blk_dst, uint32_t n, uint32_t iq)
{
    if (FMT == GPSIQ_SC16) {
        reinterpret_cast<uint32_t *>(blk_dst)[n] = iq;                      // gps.c:2842
    } else {
        // (signed char)(x >> 4) on each int16 half, arithmetic shift          gps.c:2845
        const int i16 = (int16_t) (iq & 0xffffu), q16 = (int16_t) (iq >> 16);
        reinterpret_cast<uint16_t *>(blk_dst)[n] =
            (uint16_t) (((uint32_t) (i16 >> 4) & 0xffu) | (((uint32_t) (q16 >> 4) & 0xffu) << 8));
    }
}

// the sample with the output level stage: i_acc / q_acc are the noiseless sums, zi / zq the sample's noise
template <int FMT>
__device__ __forceinline__ void store_level(uint8_t *__restrict__ blk_dst, uint32_t n, int i_acc, int q_acc, int zi, int zq,
                                            uint32_t lmult, int32_t lqmax)
{
    const uint32_t oi = (uint32_t) level::apply((int16_t) i_acc + zi, lmult, lqmax);
    const uint32_t oq = (uint32_t) level::apply((int16_t) q_acc + zq, lmult, lqmax);
    if (FMT == GPSIQ_SC16) reinterpret_cast<uint32_t *>(blk_dst)[n] = (oi & 0xffffu) | (oq << 16);
    else                   reinterpret_cast<uint16_t *>(blk_dst)[n] = (uint16_t) ((oi & 0xffu) | (oq << 8));
}

// ---------------------------------------------------------------------------
// Generic kernel: one sample per thread per step, every quantity of the closed form
// evaluated at full width for that sample.  Works for any rate the descriptor format
// allows; it is the fallback for sample rates too low for the row kernel, and an
// independent second implementation the tests cross-check the row kernel against.
template <int FMT>
__global__ __launch_bounds__(kGenericThreads) void synth_generic(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block,
    int tile_samples, const noise::Entry *__restrict__ ntab, uint64_t nseed, uint64_t nblock0, uint32_t lmult, int32_t lqmax)
{
    __shared__ uint32_t lut[kMaxChan][512];
    __shared__ uint32_t ext[kMaxChan][kPrnExtWords];
    __shared__ gpsiq_qchan_t qs[kMaxChan];

    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    stage_block<kGenericThreads>(desc + (size_t) (block0 + blk) * nchan, nchan, tab, qs, lut, ext);
    uint8_t *blk_dst = dst + (size_t) blk * block_stride;

    const uint32_t n_begin = (uint32_t) tile * (uint32_t) tile_samples;
    uint32_t n_end = n_begin + (uint32_t) tile_samples;
    if (n_end > (uint32_t) nsamp) n_end = (uint32_t) nsamp;

    // noise (ntab != nullptr): a thread keeps one lane stream (tile_samples and the stride are multiples of 64) and moves
    // kGenericThreads/64 rows per step
    uint64_t nx = 0, nA = 0, nC = 0;
    if (ntab) {
        const uint32_t n = n_begin + threadIdx.x;
        noise::jump(n >> 6, noise::kMul, noise::kInc, &nA, &nC);
        nx = nA * noise::lane_start(nseed, nblock0 + (uint64_t) (block0 + blk), n & 63u) + nC;
        noise::jump(kGenericThreads / 64, noise::kMul, noise::kInc, &nA, &nC);
    }
    for (uint32_t n = n_begin + threadIdx.x; n < n_end; n += kGenericThreads) {
        int i_acc = 0, q_acc = 0, zi = 0, zq = 0;
        if (ntab) {
            const uint32_t w = noise::xsh_rr(nx);
            nx = nA * nx + nC;
            zi = noise::z(ntab, w & 0xffffu);
            zq = noise::z(ntab, w >> 16);
        }
        for (int c = 0; c < nchan; ++c) {
            const gpsiq_qchan_t &q = qs[c];
            if (q.prn == 0) continue;
            const uint32_t idx = carrier_index(q, n);
            const uint64_t A = chip_count(q, n);
            const uint32_t chip = code_chip(A), bit = data_bit(q, A);
            const uint32_t neg = ((ext[c][chip >> 5] >> (chip & 31)) ^ (q.nav_bits >> (bit & 31))) & 1u;
            const uint32_t v = lut[c][idx];
            const int tc = (int16_t) (v & 0xffffu), ts = (int16_t) (v >> 16);
            i_acc += neg ? -tc : tc;
            q_acc += neg ? -ts : ts;
        }
        if (lmult) store_level<FMT>(blk_dst, n, i_acc, q_acc, zi, zq, lmult, lqmax);
        else store_sample<FMT>(blk_dst, n, ((uint32_t) (i_acc + zi) & 0xffffu) | ((uint32_t) (q_acc + zq) << 16));
    }
}

// ---------------------------------------------------------------------------
// Row kernel.  A "row" is 64 consecutive samples, one per lane of a wave, so that
//   * IQ stores are one contiguous 128/256-byte run per wave instruction,
//   * the carrier LUT indices of a wave are (nearly) consecutive -> conflict-free
//     ds_read_b32 with broadcasts,
//   * all lanes of a row sit inside one 32-chip window of the C/A code, a wave-uniform
//     word prepared once per (channel,row), in which a lane finds its sign with the low
//     5 bits of its own chip counter — no mod-1023, no divisions.
// Each wave owns kRowsPerWave consecutive rows.  Per channel it keeps two 64-bit
// per-lane NCO words (carrier phase, code phase) and steps them by one row with a
// 64-bit add each.  (The words and the window: gpsiq_signal.h.)
// (kWaves, kRowsPerWave and what follows from them: gpsiq_geometry.h)
constexpr int kWinRowsPerLane = kRowsPerWave * kMaxChan / 64;   // rows one lane prepares

template <int FMT>
__global__ __launch_bounds__(kRowsThreads) void synth_rows(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block)
{
    __shared__ uint32_t lut[kMaxChan][512];
    __shared__ uint32_t ext[kMaxChan][kPrnExtWords];
    __shared__ uint32_t win[kWaves][kMaxChan][kRowsPerWave];
    __shared__ gpsiq_qchan_t qs[kMaxChan];

    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    stage_block<kRowsThreads>(desc + (size_t) (block0 + blk) * nchan, nchan, tab, qs, lut, ext);
    uint8_t *blk_dst = dst + (size_t) blk * block_stride;

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n_wave = (uint32_t) tile * kRowsTile + (uint32_t) wave * (kRowsPerWave * 64);

    // ---- windows: lane (c, g) prepares rows g*R .. g*R+R-1 of channel c -----------
    {
        const int c = lane & (kMaxChan - 1), g = lane / kMaxChan;
        if (c < nchan && qs[c].prn != 0) {
            const gpsiq_qchan_t &q = qs[c];
            const uint32_t n_row = n_wave + (uint32_t) (g * kWinRowsPerLane) * 64u;
#include "gpsiq_window_setup.inc"
#pragma unroll
            for (int r = 0; r < kWinRowsPerLane; ++r) {
#include "gpsiq_window_row.inc"
                win[wave][c][g * kWinRowsPerLane + r] = window_word(S, a5);
#include "gpsiq_window_step.inc"
            }
        }
    }
    __syncthreads();

    // ---- synthesis -------------------------------------------------------------
    s16x2 acc[kRowsPerWave];
#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) acc[r] = (s16x2) (0);

    const uint32_t n0 = n_wave + (uint32_t) lane;
    for (int c = 0; c < nchan; ++c) {
        const gpsiq_qchan_t &q = qs[c];
        if (q.prn == 0) continue;
        uint64_t P = q.carr_phase + (uint64_t) q.carr_step * (uint64_t) n0;
        uint64_t Q = ((uint64_t) q.chip0 << GPSIQ_CODE_FRAC_BITS) + q.code_frac + q.code_step * (uint64_t) n0;
        const uint64_t dP = (uint64_t) q.carr_step * 64u;
        const uint64_t dQ = q.code_step * 64u;
        const unsigned char *lut_c = reinterpret_cast<const unsigned char *>(lut[c]);
        const uint32_t *win_c = win[wave][c];
#pragma unroll
        for (int r = 0; r < kRowsPerWave; ++r) {
            const uint32_t w = win_c[r];
            const uint32_t b = (uint32_t) (Q >> 56);
            const uint32_t m = (uint32_t) __builtin_amdgcn_sbfe((int) w, b, 1u);   // 0 or ~0
            const uint32_t sgn = m | 0x00010001u;                                 // (+1,+1) or (-1,-1)
            const uint32_t a = (uint32_t) (P >> 48) & 0x7fcu;                      // 4 * LUT index
            const uint32_t v = *reinterpret_cast<const uint32_t *>(lut_c + a);
            acc[r] = __builtin_bit_cast(s16x2, v) * __builtin_bit_cast(s16x2, sgn) + acc[r];
            P += dP;
            Q += dQ;
        }
    }

#pragma unroll
    for (int r = 0; r < kRowsPerWave; ++r) {
        const uint32_t n = n0 + (uint32_t) r * 64u;
        if (n < (uint32_t) nsamp)
            store_sample<FMT>(blk_dst, n, __builtin_bit_cast(uint32_t, acc[r]));
    }
}

// ---------------------------------------------------------------------------
// Row kernel, channel-inner order ("rowsx").  Same rows/windows/NCO words as synth_rows,
// but the loop nest is rows (outer) x channels (inner, fully unrolled over NCH slots):
//   * the per-lane NCO state of ALL channels stays in registers for the whole tile, so
//     the 64x32-bit start products are paid once per tile, not once per row group;
//   * the LUT base of every channel is a compile-time LDS offset (no address add);
//   * the NCH LUT gathers of a row are independent -> issued back to back, their LDS
//     latency overlaps instead of being exposed once per row;
//   * the NCH windows of a row are one contiguous 4*NCH-byte broadcast read.
// Descriptors arrive compacted (active channels first, see gpsiq_set_descriptors), the
// slots >= the block's active count are dummies: zero LUT, zero phase, zero step.
template <int FMT, int NCH>
__global__ __launch_bounds__(kRowsThreads) void synth_rowsx(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block)
{
    __shared__ uint32_t lut[NCH][512];
    __shared__ uint32_t ext[NCH][kPrnExtWords];
    __shared__ uint32_t win[kWaves][kRowsPerWave][NCH];
    __shared__ gpsiq_qchan_t qs[NCH];

    const int tid = threadIdx.x;
    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    const gpsiq_qchan_t *q_blk = desc + (size_t) (block0 + blk) * nchan;
    const int nq = nchan < NCH ? nchan : NCH;
    for (int i = tid; i < NCH * 12; i += kRowsThreads)
        reinterpret_cast<uint32_t *>(qs)[i] = i < nq * 12 ? reinterpret_cast<const uint32_t *>(q_blk)[i] : 0u;
    __syncthreads();
    for (int e = tid; e < NCH * 512; e += kRowsThreads) {
        const int c = e >> 9, k = e & 511;
        uint32_t v = 0u;
        if (qs[c].prn != 0) {
            const double g = qs[c].gain;
            const int ts = (int) ((double) dev_sin512(tab->quarter_wave, k) * g);
            const int tc = (int) ((double) dev_sin512(tab->quarter_wave, k + 128) * g);
            v = ((uint32_t) tc & 0xffffu) | ((uint32_t) ts << 16);
        }
        lut[c][k] = v;
    }
    for (int e = tid; e < NCH * kPrnExtWords; e += kRowsThreads) {
        const int c = e / kPrnExtWords, w = e % kPrnExtWords;
        ext[c][w] = qs[c].prn ? tab->prn_ext[qs[c].prn - 1][w] : 0u;
    }
    __syncthreads();
    uint8_t *blk_dst = dst + (size_t) blk * block_stride;

    const int wave = tid >> 6, lane = tid & 63;
    const uint32_t n_wave = (uint32_t) tile * kRowsTile + (uint32_t) wave * (kRowsPerWave * 64);

    // ---- windows: lane (c, g) prepares a run of consecutive rows of channel c ------
    {
        constexpr int kGroups = 64 / NCH;                   // lanes per channel
        constexpr int kRun = kRowsPerWave / kGroups;        // rows per lane
        static_assert(kRowsPerWave % kGroups == 0, "rows per wave must split over the lane groups");
        const int c = lane % NCH, g = lane / NCH;
        if (g < kGroups) {
            const gpsiq_qchan_t &q = qs[c];
            const bool on = q.prn != 0;
            const uint32_t n_row = n_wave + (uint32_t) (g * kRun) * 64u;
#include "gpsiq_window_setup.inc"
#pragma unroll 4
            for (int r = 0; r < kRun; ++r) {
#include "gpsiq_window_row.inc"
                win[wave][g * kRun + r][c] = on ? window_word(S, a5) : 0u;
#include "gpsiq_window_step.inc"
            }
        }
    }
    __syncthreads();

    // ---- per-lane NCO state of every channel --------------------------------------
    const uint32_t n0 = n_wave + (uint32_t) lane;
    uint64_t P[NCH], Q[NCH], dP[NCH], dQ[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        nco_start(q_blk, c, c < nchan, n0, &P[c], &Q[c], &dP[c], &dQ[c]);      // (the steps: 4 SGPRs per channel)

    const unsigned char *lut_b = reinterpret_cast<const unsigned char *>(&lut[0][0]);
    for (int r = 0; r < kRowsPerWave; ++r) {
        const uint32_t n = n0 + (uint32_t) r * 64u;
        if (n_wave + (uint32_t) r * 64u >= (uint32_t) nsamp) break;     // wave-uniform
        const uint32_t *w_row = win[wave][r];
        s16x2 acc0 = (s16x2) (0), acc1 = (s16x2) (0);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint32_t w = w_row[c];
            const uint32_t b = (uint32_t) (Q[c] >> 56);
            const uint32_t m = (uint32_t) __builtin_amdgcn_sbfe((int) w, b, 1u);
            const uint32_t sgn = m | 0x00010001u;
            const uint32_t a = (uint32_t) (P[c] >> 48) & 0x7fcu;
            const uint32_t v = *reinterpret_cast<const uint32_t *>(lut_b + c * 2048 + a);
            if (c & 1) acc1 = __builtin_bit_cast(s16x2, v) * __builtin_bit_cast(s16x2, sgn) + acc1;
            else       acc0 = __builtin_bit_cast(s16x2, v) * __builtin_bit_cast(s16x2, sgn) + acc0;
            P[c] += dP[c];
            Q[c] += dQ[c];
        }
        if (n < (uint32_t) nsamp)
            store_sample<FMT>(blk_dst, n, __builtin_bit_cast(uint32_t, acc0 + acc1));
    }
}

// ---------------------------------------------------------------------------
// Tile kernel ("tile"/"seg"): the row kernel in channel-inner order with the per-tile
// overhead trimmed, because the path is VALU-issue bound (profiles/r01_pmc_counters.txt:
// 9.7 VALU instructions per (channel,row) against 7 in the core):
//   * a wave owns `wave_rows` consecutive rows, worked in chunks of ROWS rows (the last chunk
//     may be partial), i.e. one contiguous run of samples:
//     the per-lane NCO words and the window-builder state simply continue from chunk to
//     chunk, so the start products, the mod-1023 / mod-20 set-up and the LUT build are
//     paid once per workgroup, not once per 64 rows ("seg": the host cuts every block into
//     equal runs of ~250 rows per wave; "tile": wave_rows = ROWS);
//   * LUT build: thread k owns LUT entry k of every channel, so sin/cos of k are formed
//     once and each entry costs two f64 multiplies and two truncations;
//   * window set-up in 32-bit chip arithmetic (a block never advances 2^32 chips);
//   * a chunk whose rows all lie inside the block runs a check-free row loop; in the plain-add cores that loop takes four
//     rows per trip and reads the next row's windows while a row is worked (gpsiq_tile_body.inc, "rows per loop trip").
//   * H = 2 ("segh"): one window per HALF row (32 lanes), so a row may span up to 63 chips
//     and the kernel works down to one chip per sample (1.023 Msps); lanes 32..63 read the
//     second window of their row (two LDS addresses per wave read instead of one).
//   * FAST (int16 output: chosen by the host when no sum over the channels of a block can leave the
//     int16 range, i.e. sum of (int)(250*|gain|) <= 32767; int8 output: always): the LUT entry is the
//     single integer I + 65536*Q (int8: two 12-bit fields), the channel sum is a plain 32-bit add
//     (exact: it cannot overflow / the fields cannot collide), and the chip
//     sign is applied as half a carrier cycle: the carrier table is antisymmetric
//     (table[k+256] == -table[k], so is (int)(table*gain)), hence adding the sign bit to the top
//     index bit of the phase word selects the negated entry.  The shifted window's higher bits land
//     in the five spare bits above the index.  lshr, lshl_add, add replace bfe, or, pk_mad.
//   * BOTH ("segb", with FAST): the LUT holds both polarities, entry sign*512 + k = entry (k + 256*sign) mod 512, so the
//     chip sign is CONCATENATED above the index instead of added to it: with the phase word kept left-aligned (index in
//     bits 23..31 of its high half) one v_alignbit_b32 puts {sign, index} at bits 2..11 and a plain v_and_b32 with a
//     literal (2.5 issue cycles, where the SDWA form it replaces takes 4.3) makes the LDS address.  The table is 4 KB per
//     channel, so a workgroup has WAVES = 16 waves (64 KB of LUT + 64 KB of windows, one workgroup per CU = the same four
//     waves per SIMD).
//   * NOISE (synth_tile_noise): receiver noise (include/gpsiq.h) added to each sample's sums before the store.  A lane owns
//     lane stream `lane` of its block and its wave's rows are consecutive, so after a wave-uniform jump to the wave's first row
//     a row costs one LCG step, xsh_rr and two gathers in the scaled table (LDS, beside the carrier LUT).  Both kernels include
//     one body (gpsiq_tile_body.inc) with NOISE a constant: the noise-off kernels keep their names and their code.
//   * LEVEL (synth_tile_level): the output level stage (include/gpsiq_rows.h) behind the noise: I and Q come out of the packed word
//     sign-extended, the noise is added in 32 bits, then multiply-add, shift and clamp per component and one packed store.  Both
//     output formats run the int16 cores (the int8 core's 12-bit fields cannot give the whole sums back).
template <int FMT, int NCH, int ROWS, int H, bool FAST, int WAVES = kWaves, bool BOTH = false>
__global__ __launch_bounds__(WAVES * 64, 4) void synth_tile(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block,
    int wave_rows, int big_wgs, int big_blocks, int tiles_small)
{
    constexpr bool NOISE = false, LEVEL = false;
    [[maybe_unused]] constexpr const noise::Entry *ntab = nullptr;
    [[maybe_unused]] constexpr uint64_t nseed = 0, nblock0 = 0;
    [[maybe_unused]] constexpr uint32_t lmult = 0;
    [[maybe_unused]] constexpr int32_t lqmax = 0;
#include "gpsiq_tile_body.inc"
}

// the same with receiver noise: ntab is the scaled table (noise::kTabEntries entries), nblock0 the absolute index of desc's block 0
template <int FMT, int NCH, int ROWS, int H, bool FAST>
__global__ __launch_bounds__(kWaves * 64, 4) void synth_tile_noise(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block,
    int wave_rows, int big_wgs, int big_blocks, int tiles_small,
    const noise::Entry *__restrict__ ntab, uint64_t nseed, uint64_t nblock0)
{
    constexpr int WAVES = kWaves;
    constexpr bool BOTH = false, NOISE = true, LEVEL = false;
    [[maybe_unused]] constexpr uint32_t lmult = 0;
    [[maybe_unused]] constexpr int32_t lqmax = 0;
#include "gpsiq_tile_body.inc"
}

// the same with the output level stage behind the noise (include/gpsiq_rows.h): lmult / 65536 is the scale, lqmax the clamp.  While
// the noise is off ntab is an all-zero table (the host's choice).  FAST here means the int16 plain-add core, for
// either output format.
template <int FMT, int NCH, int ROWS, int H, bool FAST>
__global__ __launch_bounds__(kWaves * 64, 4) void synth_tile_level(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, int tiles_per_block,
    int wave_rows, int big_wgs, int big_blocks, int tiles_small,
    const noise::Entry *__restrict__ ntab, uint64_t nseed, uint64_t nblock0, uint32_t lmult, int32_t lqmax)
{
    constexpr int WAVES = kWaves;
    constexpr bool BOTH = false, NOISE = true, LEVEL = true;
#include "gpsiq_tile_body.inc"
}

// ---------------------------------------------------------------------------
// Mask kernels ("segm"): an experiment for high sample rates, kept as a selectable, parity-tested variant; NOT the
// default, because it measured slower than seg (the row loop itself reaches its instruction
// count -- 0.78 ms against seg's 1.43 ms per 2 GiB at 25 Msps -- but delivering one 64-bit mask per (channel, row)
// costs more than it saves: +0.74 ms for streaming them through the scalar cache, +0.44 ms for the pre-pass).
// The idea: at >= 8 Msps a row of 64 samples holds only a few chip edges,
// so the chip-sign of a (channel, row) is a 64-bit lane mask that ONE thread can build bit-parallel by walking
// the edges with an exact DDA (sign_masks, a pre-pass: about ten instructions per edge, 64 (channel, row)s per
// wave instruction).  The row loop then needs no code NCO and no window per lane: the mask arrives through a
// scalar load as an EXEC mask, and the sign is applied as half a carrier cycle by one exec-masked
// v_xor_b32 a, 0x400, a on the LDS address (a plain two-operand VALU form).  Per (channel, row): carrier NCO add,
// SDWA and (address), masked xor, 1/2 add3 = 3.5 VALU instructions instead of 5.5, and nothing but the carrier
// LUT in LDS.  The arithmetic is the closed form of include/gpsiq.h, evaluated exactly:
//   sample pos of the chip edge e of a row: smallest pos with  f0 + pos*cs >= e*2^56  (f0: code fraction at the
//   row start), walked with  2^56 = q*cs + r:  the next edge is q or q+1 samples on, by the remainder.
__global__ __launch_bounds__(kMaskThreads) void sign_masks(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, int block0, int nblocks,
    const DeviceTables *__restrict__ tab, uint64_t *__restrict__ masks, int rows_total, int rowgroups)
{
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = (int) (t & 15u);
    const unsigned g = t >> 4;
    const int rg = (int) (g % (unsigned) rowgroups), blk = (int) (g / (unsigned) rowgroups);
    if (blk >= nblocks) return;
    const int row0 = rg * kMaskRowsPerThread;
    uint64_t *out = masks + ((size_t) blk * rows_total + row0) * 16 + c;
    int nrows = rows_total - row0;
    if (nrows > kMaskRowsPerThread) nrows = kMaskRowsPerThread;
    if (c >= nchan || desc[(size_t) (block0 + blk) * nchan + c].prn == 0) {     // unused slot: its LUT is all zero
        for (int r = 0; r < nrows; ++r) out[(size_t) r * 16] = 0u;
        return;
    }
    const gpsiq_qchan_t q = desc[(size_t) (block0 + blk) * nchan + c];
    const uint32_t *prn = tab->prn_ext[q.prn - 1];
    const uint64_t cs = q.code_step;
    const unsigned __int128 T = (unsigned __int128) q.code_frac + (unsigned __int128) cs * (unsigned) (row0 * 64);
    const uint32_t A0 = (uint32_t) q.chip0 + (uint32_t) (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
    const uint64_t f0 = (uint64_t) T & kCodeFracMask;
    uint32_t k = A0 % GPSIQ_CA_SEQ_LEN;
    const uint32_t ic = q.icode + A0 / GPSIQ_CA_SEQ_LEN;
    uint32_t bit = ic / 20u, icur = ic % 20u;
    const uint64_t one = UINT64_C(1) << GPSIQ_CODE_FRAC_BITS;
    const uint64_t q56 = one / cs, r56 = one % cs;
    // first edge after the group's first sample: smallest pos with f0 + pos*cs >= 2^56
    const uint64_t d = one - f0;
    uint64_t pos = (d + cs - 1) / cs;
    uint64_t over = pos * cs - d;                         // how far past the edge that sample is, < cs
    uint32_t sgn = ((prn[k >> 5] >> (k & 31u)) ^ (q.nav_bits >> (bit & 31u))) & 1u;
    for (int r = 0; r < nrows; ++r) {
        uint64_t m = sgn ? ~UINT64_C(0) : UINT64_C(0);
        while (pos < 64u) {
            if (++k == GPSIQ_CA_SEQ_LEN) {                 // gps.c:2791-2811: next code period, maybe next data bit
                k = 0;
                if (++icur == 20u) { icur = 0; ++bit; }
            }
            const uint32_t ns = ((prn[k >> 5] >> (k & 31u)) ^ (q.nav_bits >> (bit & 31u))) & 1u;
            if (ns != sgn) { m ^= ~UINT64_C(0) << pos; sgn = ns; }
            if (r56 > over) { pos += q56 + 1; over += cs - r56; }
            else            { pos += q56;     over -= r56; }
        }
        out[(size_t) r * 16] = m;
        pos -= 64u;
    }
}

template <int FMT, int NCH>
__global__ __launch_bounds__(kRowsThreads) void synth_mask(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst,
    size_t block_stride, int block0, const DeviceTables *__restrict__ tab, const uint64_t *__restrict__ masks,
    int rows_total, int tiles_per_block, int wave_rows)
{
    __shared__ uint32_t lut[NCH][512];
    __shared__ gpsiq_qchan_t qs[NCH];
    const int tid = threadIdx.x;
    const int blk = blockIdx.x / tiles_per_block, tile = blockIdx.x % tiles_per_block;
    const gpsiq_qchan_t *q_blk = desc + (size_t) (block0 + blk) * nchan;
    const int nq = nchan < NCH ? nchan : NCH;
    for (int i = tid; i < NCH * 12; i += kRowsThreads)
        reinterpret_cast<uint32_t *>(qs)[i] = i < nq * 12 ? reinterpret_cast<const uint32_t *>(q_blk)[i] : 0u;
    __syncthreads();
    {
        const double sk = (double) dev_sin512(tab->quarter_wave, tid);
        const double ck = (double) dev_sin512(tab->quarter_wave, tid + 128);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const double g = qs[c].gain;
            const int ts = (int) (sk * g), tc = (int) (ck * g);   // gps.c:2781-2782
            // the plain-add formats of synth_tile<FAST>: int8 two 12-bit fields, int16 one integer with slot 0's bias
            if (FMT == GPSIQ_SC08) lut[c][tid] = (((uint32_t) tc & 0xfffu) << 4) | ((uint32_t) ts << 20);
            else                   lut[c][tid] = (uint32_t) (tc + ts * 65536) + (c == 0 ? 0x8000u : 0u);
        }
    }
    __syncthreads();
    uint8_t *blk_dst = dst + (size_t) blk * block_stride;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int row_first = (tile * kWaves + wave) * wave_rows;
    if (row_first >= rows_total) return;
    int rows = rows_total - row_first;
    rows = rows < wave_rows ? rows : wave_rows;
    const uint32_t n0 = (uint32_t) row_first * 64u + (uint32_t) lane;
    uint64_t P[NCH], dP[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const bool have = c < nchan;
        const uint64_t p0 = have ? q_blk[c].carr_phase : 0u, ps = have ? (uint64_t) q_blk[c].carr_step : 0u;
        P[c] = p0 + ps * (uint64_t) n0;
        dP[c] = ps * 64u;
    }
    const unsigned char *lut_b = reinterpret_cast<const unsigned char *>(&lut[0][0]);
    // the 16 masks of a row are one 128-byte line at a wave-uniform address: two s_load_dwordx16 per row
    typedef uint64_t u64x8 __attribute__((ext_vector_type(8)));
    const u64x8 *m_row = reinterpret_cast<const u64x8 *>(masks + ((size_t) blk * rows_total + row_first) * 16);
    const int rows_s = __builtin_amdgcn_readfirstlane(rows);
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int r = 0; r < rows_s; ++r) {
        const u64x8 m_lo = m_row[2 * r];
        u64x8 m_hi = m_lo;
        if (NCH > 8) m_hi = m_row[2 * r + 1];
        uint32_t sum = 0u;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const uint64_t m = c < 8 ? m_lo[c] : m_hi[c - 8];
            uint32_t a = (uint32_t) (P[c] >> 48) & 0x7fcu;                      // 4 * LUT index
            uint64_t saved;
            // lanes whose chip sign is -1 read the entry half a cycle on: the table is antisymmetric
            asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\tv_xor_b32 %[a], 0x400, %[a]\n\ts_mov_b64 exec, %[sv]"
                         : [a] "+v"(a), [sv] "=&s"(saved) : [m] "s"(m));
            sum += *reinterpret_cast<const uint32_t *>(lut_b + c * 2048 + a);
            P[c] += dP[c];
        }
        const uint32_t iq = FMT == GPSIQ_SC16 ? sum ^ 0x8000u : sum;
        const uint32_t n = n0 + (uint32_t) r * 64u;
        if (n < (uint32_t) nsamp) {
            if (FMT == GPSIQ_SC16) *reinterpret_cast<uint32_t *>(blk_dst + n * 4u) = iq;
            else *reinterpret_cast<uint16_t *>(blk_dst + n * 2u) = (uint16_t) __builtin_amdgcn_perm(iq, iq, 0x0c0c0301u);
        }
    }
}

// ---------------------------------------------------------------------------
// GPSIQ_NCO_REFERENCE fix-up (csrc/gpsiq_exact.cpp): the few samples per 10^7 where the reference's
// double accumulators pick another LUT entry or sign than the closed form are recomputed whole --
// every channel from the closed form, the patched channels from the patch -- and stored over what
// the synthesis kernel wrote (same stream, after it).  Sixteen lanes per patch, one channel each (the
// closed form of one channel is a chain of 128-bit products and a division: sixteen of them one
// after the other in one thread were 13-18 us of a 200 us piece), summed with cross-lane
// shuffles inside each group of sixteen; the first patch of a (block, sample) group does the sample, lane 0 stores it.
template <int FMT>
__global__ __launch_bounds__(64) void apply_patches(
    const gpsiq_qchan_t *__restrict__ desc, int nchan, int nsamp, uint8_t *__restrict__ dst, size_t block_stride,
    int block0, int nblocks, const DeviceTables *__restrict__ tab, const gpsiq_patch_t *__restrict__ pt, int npatch,
    const noise::Entry *__restrict__ ntab, uint64_t nseed, uint64_t nblock0, uint32_t lmult, int32_t lqmax)
{
    const int i = (int) (blockIdx.x * 4u + (threadIdx.x >> 4));      // four patches per wave
    const int c = (int) (threadIdx.x & 15u);                          // this lane's channel slot (GPSIQ_MAX_CHAN = 16)
    const bool have = i < npatch;
    const gpsiq_patch_t p = pt[have ? i : npatch - 1];
    bool lead = have && !(i > 0 && pt[i - 1].block == p.block && pt[i - 1].sample == p.sample);
    lead = lead && p.block >= (uint32_t) block0 && p.block < (uint32_t) (block0 + nblocks) && p.sample < (uint32_t) nsamp;
    int i_acc = 0, q_acc = 0;
    if (lead && c < nchan) {
        const gpsiq_qchan_t qc = desc[(size_t) p.block * nchan + c];
        if (qc.prn != 0) {
            const uint64_t n = p.sample;
            // (the closed form of gpsiq_signal.h, written out: with its functions this kernel's instruction stream moves)
            const uint64_t P = qc.carr_phase + (uint64_t) qc.carr_step * n;
            uint32_t idx = (uint32_t) (P >> (GPSIQ_CARR_FRAC_BITS - 9)) & 511u;
            const unsigned __int128 T = (unsigned __int128) qc.code_frac + (unsigned __int128) qc.code_step * (unsigned __int128) n;
            const uint64_t A = (uint64_t) qc.chip0 + (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
            const uint32_t chip = (uint32_t) (A % GPSIQ_CA_SEQ_LEN);
            const uint32_t bit = (uint32_t) ((qc.icode + A / GPSIQ_CA_SEQ_LEN) / 20);
            uint32_t neg = ((tab->prn_ext[qc.prn - 1][chip >> 5] >> (chip & 31)) ^ (qc.nav_bits >> (bit & 31))) & 1u;
            for (int j = i; j < npatch && pt[j].block == p.block && pt[j].sample == p.sample; ++j)
                if (pt[j].slot == c) { idx = pt[j].lut & 511u; neg = pt[j].neg & 1u; }
            const int ts = (int) ((double) dev_sin512(tab->quarter_wave, (int) idx) * qc.gain);        // gps.c:2782
            const int tc = (int) ((double) dev_sin512(tab->quarter_wave, (int) idx + 128) * qc.gain);  // gps.c:2781
            i_acc = neg ? -tc : tc;
            q_acc = neg ? -ts : ts;
        }
    }
    // sum over the sixteen lanes of the patch (all 64 lanes take part: no divergence around the cross-lane moves)
    for (int off = 8; off >= 1; off >>= 1) {
        i_acc += __shfl_xor(i_acc, off, 16);
        q_acc += __shfl_xor(q_acc, off, 16);
    }
    int32_t zi = 0, zq = 0;
    if (lead && c == 0 && ntab)                                       // the sample's noise, as the synthesis kernel added it
        noise::sample(ntab, nseed, nblock0 + p.block, p.sample, &zi, &zq);
    if (lead && c == 0) {
        uint8_t *blk_dst = dst + (size_t) (p.block - (uint32_t) block0) * block_stride;
        if (lmult) store_level<FMT>(blk_dst, p.sample, i_acc, q_acc, zi, zq, lmult, lqmax);                // ... and the level stage
        else store_sample<FMT>(blk_dst, p.sample, ((uint32_t) (i_acc + zi) & 0xffffu) | ((uint32_t) (q_acc + zq) << 16));
    }
}

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what the launcher (gpsiq_launch.cpp) looks up with the run-time values of a plan
// (gpsiq_launch_plan.h).  Every instantiation of the library is named here and nowhere else; nullptr: no such kernel.
template <int... N> struct Ints {};
using Slots = Ints<4, 8, 12, 16>;       // channel slots of the tile, mask and both-polarity kernels
using SlotsX = Ints<4, 8, 16>;          // ... of synth_rowsx

template <int... N> constexpr int index_of(Ints<N...>, int n)
{
    int at = -1, i = 0;
    ((at = N == n ? i : at, ++i), ...);
    return at;
}
// the table of format `fmt` out of (int8, int16); its entry `i`, nullptr when i < 0
template <class T> static auto pick(const T &t08, const T &t16, int fmt, int i) -> typename T::value_type
{
    return i < 0 || (fmt != GPSIQ_SC08 && fmt != GPSIQ_SC16) ? nullptr : (fmt == GPSIQ_SC16 ? t16 : t08)[(size_t) i];
}

// tile / seg (64 rows per chunk, a window per row) and segh (32 rows, two windows per row), packed and plain-add core, per family
struct Plain { template <int F, int N, int R, int H, bool FA> static constexpr TileFn      fn = synth_tile<F, N, R, H, FA>; };
struct Noise { template <int F, int N, int R, int H, bool FA> static constexpr TileNoiseFn fn = synth_tile_noise<F, N, R, H, FA>; };
struct Level { template <int F, int N, int R, int H, bool FA> static constexpr TileLevelFn fn = synth_tile_level<F, N, R, H, FA>; };

template <class K, int F, int... N> constexpr auto tile_fns(Ints<N...>)
{
    using Fn = std::remove_const_t<decltype(K::template fn<F, 4, 64, 1, false>)>;
    return std::array<Fn, 4 * sizeof...(N)>{K::template fn<F, N, 64, 1, false>..., K::template fn<F, N, 64, 1, true>...,
                                            K::template fn<F, N, 32, 2, false>..., K::template fn<F, N, 32, 2, true>...};
}
template <class K> static auto tile_lookup(int fmt, int slots, bool half, bool fast)
{
    static constexpr auto t08 = tile_fns<K, GPSIQ_SC08>(Slots{}), t16 = tile_fns<K, GPSIQ_SC16>(Slots{});
    const int s = index_of(Slots{}, slots);
    return pick(t08, t16, fmt, s < 0 ? -1 : ((half ? 2 : 0) + (fast ? 1 : 0)) * 4 + s);
}
TileFn      tile_kernel(int fmt, int slots, bool half, bool fast) { return tile_lookup<Plain>(fmt, slots, half, fast); }
TileNoiseFn tile_noise_kernel(int fmt, int slots, bool half, bool fast) { return tile_lookup<Noise>(fmt, slots, half, fast); }
TileLevelFn tile_level_kernel(int fmt, int slots, bool half, bool fast) { return tile_lookup<Level>(fmt, slots, half, fast); }

template <int F, int... N> constexpr std::array<TileFn, sizeof...(N)> both_fns(Ints<N...>) { return {synth_tile<F, N, both_rows(N), 1, true, kWaves, true>...}; }
template <int F, int... N> constexpr std::array<MaskFn, sizeof...(N)> mask_fns(Ints<N...>) { return {synth_mask<F, N>...}; }
template <int F, int... N> constexpr std::array<RowsFn, sizeof...(N)> rowsx_fns(Ints<N...>) { return {synth_rowsx<F, N>...}; }

TileFn both_kernel(int fmt, int slots)
{
    static constexpr auto t08 = both_fns<GPSIQ_SC08>(Slots{}), t16 = both_fns<GPSIQ_SC16>(Slots{});
    return pick(t08, t16, fmt, index_of(Slots{}, slots));
}
MaskFn mask_kernel(int fmt, int slots)
{
    static constexpr auto t08 = mask_fns<GPSIQ_SC08>(Slots{}), t16 = mask_fns<GPSIQ_SC16>(Slots{});
    return pick(t08, t16, fmt, index_of(Slots{}, slots));
}
RowsFn rowsx_kernel(int fmt, int slots)
{
    static constexpr auto t08 = rowsx_fns<GPSIQ_SC08>(SlotsX{}), t16 = rowsx_fns<GPSIQ_SC16>(SlotsX{});
    return pick(t08, t16, fmt, index_of(SlotsX{}, slots));
}
RowsFn      rows_kernel(int fmt) { return fmt == GPSIQ_SC16 ? synth_rows<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? synth_rows<GPSIQ_SC08> : nullptr; }
GenericFn   generic_kernel(int fmt) { return fmt == GPSIQ_SC16 ? synth_generic<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? synth_generic<GPSIQ_SC08> : nullptr; }
PatchFn     patch_kernel(int fmt) { return fmt == GPSIQ_SC16 ? apply_patches<GPSIQ_SC16> : fmt == GPSIQ_SC08 ? apply_patches<GPSIQ_SC08> : nullptr; }
SignMasksFn sign_masks_kernel() { return sign_masks; }
}  // namespace gpsiq
