// gpsiq_signal.h -- the device side of the signal model of include/gpsiq.h, stated once for every kernel file: the carrier table, the
// stream sample, the closed form of one sample and the NCO words that the synthesis, the correlator and the acquisition search share.
// The 32-chip sign window walker belongs here too; it is textual (gpsiq_window_setup.inc, _row.inc and _step.inc, for the reason at
// the top of gpsiq_tile_body.inc) and is explained below, with the words it works on.
// A piece lives here only in a form that leaves every kernel's instruction stream as it was (scripts/row_loop_listing.py --hashes).
// Where no form did, the site keeps its own text: the closed form in apply_patches, the carrier half of nco_start in synth_mask, and
// the descriptor and code staging loops of the row kernels.
#ifndef GPSIQ_SIGNAL_H
#define GPSIQ_SIGNAL_H

#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"

namespace gpsiq {

constexpr uint64_t kCodeFracMask = (UINT64_C(1) << GPSIQ_CODE_FRAC_BITS) - 1;
constexpr uint64_t kCarrFracMask = (UINT64_C(1) << GPSIQ_CARR_FRAC_BITS) - 1;

// sinTable512[k] from its first quarter wave (gpsiq_tables.h: sin[k] = sin[255 - k], sin[k + 256] = -sin[k]); cos[k] = sin[k + 128]
__device__ __forceinline__ int dev_sin512(const int16_t *qw, int k)
{
    k &= 511;
    int h = k & 255;
    int v = qw[h < 128 ? h : 255 - h];
    return k < 256 ? v : -v;
}

// the unit table: entry k = cosTable512[k] | sinTable512[k] << 16, what (int)(table * 1.0) gives.  NT threads, no barrier.
template <int NT>
__device__ __forceinline__ void stage_unit(const DeviceTables *__restrict__ tab, uint32_t *unit)
{
    for (int k = threadIdx.x; k < 512; k += NT)
        unit[k] = ((uint32_t) dev_sin512(tab->quarter_wave, k + 128) & 0xffffu) | ((uint32_t) dev_sin512(tab->quarter_wave, k) << 16);
}

// sample n of a stream as stored (no << 4 for int8).  A lane with valid == false reads nothing and gets (0, 0): bytes past the end of
// a block never enter a sum.
template <int FMT, class Index>
__device__ __forceinline__ void load_iq(const uint8_t *__restrict__ src, Index n, int *i, int *q, bool valid = true)
{
    *i = 0; *q = 0;
    if (!valid) return;
    if (FMT == GPSIQ_SC16) {
        const uint32_t v = reinterpret_cast<const uint32_t *>(src)[n];
        *i = (int16_t) (v & 0xffffu); *q = (int32_t) v >> 16;
    } else {
        const uint32_t v = reinterpret_cast<const uint16_t *>(src)[n];
        *i = (int8_t) (v & 0xffu); *q = (int8_t) (v >> 8);
    }
}

// The closed form of sample n of one channel at full width: carrier table index, absolute chip count A, and from A the chip inside
// the code period and the data bit.  The sign of the sample is (code chip) xor (nav_bits >> (bit & 31)); where the code is read
// from is the caller's.
__device__ __forceinline__ uint32_t carrier_index(const gpsiq_qchan_t &q, uint64_t n)
{
    const uint64_t P = q.carr_phase + (uint64_t) q.carr_step * n;
    return (uint32_t) (P >> (GPSIQ_CARR_FRAC_BITS - 9)) & 511u;
}
__device__ __forceinline__ uint64_t chip_count(const gpsiq_qchan_t &q, uint64_t n)
{
    const unsigned __int128 T = (unsigned __int128) q.code_frac + (unsigned __int128) q.code_step * (unsigned __int128) n;
    return (uint64_t) q.chip0 + (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
}
__device__ __forceinline__ uint32_t code_chip(uint64_t A) { return (uint32_t) (A % GPSIQ_CA_SEQ_LEN); }
__device__ __forceinline__ uint32_t data_bit(const gpsiq_qchan_t &q, uint64_t A) { return (uint32_t) ((q.icode + A / GPSIQ_CA_SEQ_LEN) / 20); }

// The NCO words of the row kernels.  A row is 64 consecutive samples, one per lane; per channel a lane keeps
//   the carrier word  [5 don't-care][table index : 9][fraction : 50]
//   the code word     [chips mod 256 : 8][fraction : 56]
// and steps each by one row with a 64-bit add.  The start values at the lane's first sample n0 are exact: 64x32-bit products that wrap
// mod 2^64 = mod 32 cycles / mod 256 chips.  The descriptor fields come through scalar loads (uniform address, read-only global): the
// row steps must live in SGPRs, or they cost VGPRs per channel.  have == false (a slot past the block's descriptors): all zero.
__device__ __forceinline__ void nco_start(const gpsiq_qchan_t *q_blk, int c, bool have, uint32_t n0, uint64_t *P, uint64_t *Q, uint64_t *dP, uint64_t *dQ)
{
    const uint64_t p0 = have ? q_blk[c].carr_phase : 0u, ps = have ? (uint64_t) q_blk[c].carr_step : 0u;
    const uint64_t f0 = have ? q_blk[c].code_frac : 0u, cs = have ? q_blk[c].code_step : 0u;
    const uint64_t c0 = have ? (uint64_t) q_blk[c].chip0 : 0u;
    *P = p0 + ps * (uint64_t) n0;
    *Q = (c0 << GPSIQ_CODE_FRAC_BITS) + f0 + cs * (uint64_t) n0;
    *dP = ps * 64u;
    *dQ = cs * 64u;
}

// The sign window.  All lanes of a row sit inside one 32-chip window of the C/A code, which is a wave-uniform 32-bit word W (chip xor
// data bit) prepared once per (channel, row): W[A mod 32] is the sign of absolute chip A, so a lane needs only the low 5 bits of the
// chip count in its code word to find its sign -- no mod-1023, no division.  A builder lane walks consecutive rows of one channel:
//   gpsiq_window_setup.inc   from the descriptor `q` and the first sample `n_row` of the lane's first row: the chip inside the period
//                            k, the data bit and the period inside it (bit, icur), A mod 32 (a5), the fraction and the row step
//   gpsiq_window_row.inc     S, the signs of the current row's window in code order: 32 chips from chip k of the wrap-extended code
//                            ext[c], the chips past the end of the period under the NEXT period's data bit
//   window_word(S, a5)       W: S turned so that chip A sits at bit A mod 32
//   gpsiq_window_step.inc    on by one row (less than 32 chips: one period wrap at most), with the period and data-bit wrap
// The loop, its bound and unroll pragma, where W is stored and what an unused slot gets stay with the kernel.
__device__ __forceinline__ uint32_t window_word(uint32_t S, uint32_t a5) { return __builtin_rotateleft32(S, a5 & 31u); }

}  // namespace gpsiq
#endif
