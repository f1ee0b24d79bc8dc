// gpsiq_pack_kernels.hip -- gfx950 (MI355X, wave64) kernels of gpsiq_pack / gpsiq_unpack (include/gpsiq_rows.h, "Packed streams"):
// a rendered device stream (interleaved I,Q, int8 or int16, block b at src + b * stride) to and from the packed 4- and 2-bit
// formats.  Pure byte streams: no table, no NCO, no LDS beyond the four partial counts of a workgroup.
//   pack_stream<SRC_FMT, BITS>     clamps every element to the field range (+-7 / +-1, symmetric), counts the elements it had to
//                                  clamp and inserts the two's-complement fields, I in the low bits
//   unpack_stream<BITS, DST_FMT>   sign-extends the fields into int8 / int16 elements, no shift
// A lane works on UNITS (gpsiq_pack_geometry.h): pack loads 2 or 4 x 16 consecutive source bytes and stores 16 packed bytes (8 for
// int16 -> 2 bit) at once, unpack loads 16 packed bytes and stores 32 .. 128 bytes of elements 16 at a time.  Block bases are
// 4-byte aligned and no more (src + b * stride), so every wide access is declared with 4-byte alignment: the dword form, which
// global memory serves at any dword address.  A unit is wide only where ALL of it lies inside the block's own length; the one
// ragged unit at a block's end goes element by element, bounded by 2 * nsamp and by the packed length -- never by the stride: a
// byte between or behind the blocks is neither read nor written.
// Clamp, test and field insertion work on whole dwords: the elements as packed 16-bit pairs (v_pk_max_i16 / v_pk_min_i16 clamp two
// at once, int8 elements are first split into their I and Q pairs by two packed shifts), the test is the packed XOR of before and
// after, the fields are masked and shifted a dword at a time and gathered with v_perm_b32.
#include <hip/hip_runtime.h>

#include "gpsiq_ctx.h"
#include "gpsiq_pack_geometry.h"

namespace gpsiq {
namespace {

typedef short pk_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short pk_u16x2 __attribute__((ext_vector_type(2)));
struct Quad { uint32_t w[4]; };

// 16 / 8 bytes at a 4-byte aligned address
__device__ __forceinline__ Quad load16(const uint8_t *p)
{
    Quad v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 16);
    return v;
}
__device__ __forceinline__ void store16(uint8_t *p, const Quad &v) { __builtin_memcpy(__builtin_assume_aligned(p, 4), &v, 16); }
__device__ __forceinline__ void store8(uint8_t *p, uint32_t a, uint32_t b)
{
    const uint32_t v[2] = {a, b};
    __builtin_memcpy(__builtin_assume_aligned(p, 4), v, 8);
}

// two elements at once: clamp to +-QMAX, and add 2 to the matching half of acc for every element that changed.  An element and its
// clamped value have the same sign, so bit 15 of their XOR is clear and the XOR doubled stays inside its half: 0 where nothing
// changed, at least 2 where something did, and one packed unsigned minimum with 2 makes the flag
template <int QMAX>
__device__ __forceinline__ uint32_t clamp2(uint32_t x, pk_u16x2 &acc)
{
    const pk_s16x2 v = __builtin_bit_cast(pk_s16x2, x);
    pk_s16x2 c = __builtin_elementwise_min(v, (pk_s16x2) (short) QMAX);
    // (max(c, -1) is c | c >> 15, and stays a packed operation written that way)
    c = QMAX == 1 ? c | (c >> 15) : __builtin_elementwise_max(c, (pk_s16x2) (short) -QMAX);
    const uint32_t twice = (x ^ __builtin_bit_cast(uint32_t, c)) << 1;
    acc += __builtin_elementwise_min(__builtin_bit_cast(pk_u16x2, twice), (pk_u16x2) (unsigned short) 2);
    return __builtin_bit_cast(uint32_t, c);
}

// the low bytes of four dwords as one
__device__ __forceinline__ uint32_t bytes4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3)
{
    return __builtin_amdgcn_perm(b1, b0, 0x0c0c0400u) | __builtin_amdgcn_perm(b3, b2, 0x04000c0cu);
}

// 16 source bytes -> 16 / sample_size * BITS / 8 packed bytes, in out[0 .. ]'s low bytes upward
//   int8 -> 4 bit: out[0], out[1]      int8 -> 2 bit, int16 -> 4 bit: out[0]      int16 -> 2 bit: the low half of out[0]
template <int FMT, int BITS>
__device__ __forceinline__ void pack16(const Quad &s, uint32_t *out, pk_u16x2 &acc)
{
    constexpr int QMAX = BITS == 4 ? 7 : 1;
    constexpr uint32_t kField = BITS == 4 ? 0x000f000fu : 0x00030003u;
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (FMT == GPSIQ_SC08) {
            // I0 Q0 I1 Q1 in one dword: the I pair and the Q pair, sign-extended to 16 bits
            const pk_u16x2 x = __builtin_bit_cast(pk_u16x2, s.w[k]);
            const uint32_t e = clamp2<QMAX>(__builtin_bit_cast(uint32_t, __builtin_bit_cast(pk_s16x2, x << 8) >> 8), acc);
            const uint32_t o = clamp2<QMAX>(__builtin_bit_cast(uint32_t, __builtin_bit_cast(pk_s16x2, x) >> 8), acc);
            t[k] = (e & kField) | ((o & kField) << BITS);          // sample 0's fields from bit 0, sample 1's from bit 16
            if (BITS == 2) t[k] |= t[k] >> 12;                     // 2 bit: both samples' nibbles in the low byte
        } else {
            // I Q of one sample in one dword
            const uint32_t c = clamp2<QMAX>(s.w[k], acc) & kField;
            t[k] = c | (c >> (16 - BITS));                         // the sample's fields from bit 0
        }
    }
    if (FMT == GPSIQ_SC08 && BITS == 4) {
        out[0] = __builtin_amdgcn_perm(t[1], t[0], 0x06040200u);   // bytes 0 and 2 of each
        out[1] = __builtin_amdgcn_perm(t[3], t[2], 0x06040200u);
    } else if (FMT == GPSIQ_SC16 && BITS == 2) {
        const uint32_t lo = t[0] | (t[1] << 4), hi = t[2] | (t[3] << 4);     // a nibble per sample: two samples per byte
        out[0] = __builtin_amdgcn_perm(hi, lo, 0x0c0c0400u);
    } else {
        out[0] = bytes4(t[0], t[1], t[2], t[3]);
    }
}

template <int FMT>
__device__ __forceinline__ int load_elem(const uint8_t *blk, uint64_t e)
{
    return FMT == GPSIQ_SC16 ? (int) reinterpret_cast<const int16_t *>(blk)[e] : (int) reinterpret_cast<const int8_t *>(blk)[e];
}

// Arguments: source stream and its block stride, destination and its block stride, samples per block, units per block, tiles per
// block, tiles of the launch (gpsiq_pack_plan.h), the counter (zeroed by the host).
template <int FMT, int BITS>
__global__ __launch_bounds__(kPackThreads) void pack_stream(const uint8_t *__restrict__ src, size_t src_stride, uint8_t *__restrict__ dst,
                                                             size_t dst_stride, int nsamp, uint32_t units, uint32_t tiles, uint64_t total,
                                                             unsigned long long *__restrict__ count)
{
    constexpr int LOADS = pack_unit_loads(FMT, BITS), SRC = pack_unit_src_bytes(FMT, BITS), DST = pack_unit_dst_bytes(FMT, BITS);
    constexpr int OUT = DST / LOADS;                                  // packed bytes per 16 source bytes: 8, 4, 4, 2
    constexpr int QMAX = BITS == 4 ? 7 : 1, FIELDS = 8 / BITS;
    const uint64_t nelem = (uint64_t) 2 * (uint64_t) (uint32_t) nsamp, src_len = nelem * FMT;
    const uint64_t dst_len = BITS == 4 ? (uint64_t) (uint32_t) nsamp : ((uint64_t) (uint32_t) nsamp + 1) / 2;
    uint64_t clipped = 0;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint64_t blk = w / tiles;
        const uint32_t tile = (uint32_t) (w - blk * tiles);
        const uint8_t *bs = src + blk * src_stride;
        uint8_t *bd = dst + blk * dst_stride;
#pragma unroll
        for (int j = 0; j < kPackUnitsPerThread; ++j) {
            const uint64_t u = ((uint64_t) tile * kPackUnitsPerThread + j) * kPackThreads + threadIdx.x;
            if (u >= units) continue;
            if ((u + 1) * SRC <= src_len) {                           // all of the unit is the block's: DST packed bytes follow
                pk_u16x2 acc = (pk_u16x2) (unsigned short) 0;
                Quad in[LOADS];
#pragma unroll
                for (int k = 0; k < LOADS; ++k) in[k] = load16(bs + u * SRC + 16 * k);
                uint32_t o[LOADS][2];
#pragma unroll
                for (int k = 0; k < LOADS; ++k) pack16<FMT, BITS>(in[k], o[k], acc);
                if constexpr (OUT == 8) store16(bd + u * DST, Quad{{o[0][0], o[0][1], o[1][0], o[1][1]}});
                else if constexpr (OUT == 4) store16(bd + u * DST, Quad{{o[0][0], o[1][0], o[2][0], o[3][0]}});
                else store8(bd + u * DST, o[0][0] | (o[1][0] << 16), o[2][0] | (o[3][0] << 16));
                clipped += ((uint32_t) acc.x + (uint32_t) acc.y) >> 1;       // (at most 2 * 64 per half: no carry)
            } else {
                // the ragged end of the block, a byte at a time: elements below 2 * nsamp, bytes below the packed length
                for (uint64_t b = u * DST; b < dst_len; ++b) {
                    uint32_t byte = 0;
#pragma unroll
                    for (int f = 0; f < FIELDS; ++f) {
                        const uint64_t e = b * FIELDS + f;
                        if (e >= nelem) break;                        // odd nsamp at 2 bits: the high nibble stays 0
                        const int v = load_elem<FMT>(bs, e);
                        const int c = v < -QMAX ? -QMAX : v > QMAX ? QMAX : v;
                        clipped += c != v;
                        byte |= ((uint32_t) c & ((1u << BITS) - 1)) << (f * BITS);
                    }
                    bd[b] = (uint8_t) byte;
                }
            }
        }
    }
    // count_clipped's steps (gpsiq_stream.h), kept in place: calling the shared one changes this kernel's code object
    for (int off = 32; off >= 1; off >>= 1) clipped += __shfl_xor(clipped, off, 64);
    __shared__ unsigned long long part[kPackThreads / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = clipped;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int k = 0; k < kPackThreads / 64; ++k) sum += part[k];
        if (sum) atomicAdd(count, sum);
    }
}

__device__ __forceinline__ int field_of(uint32_t x, int pos, int bits) { return (int32_t) (x << (32 - pos - bits)) >> (32 - bits); }

// one packed dword -> 32 / BITS elements, as DST_FMT * 8 / BITS dwords
template <int BITS, int FMT>
__device__ __forceinline__ void unpack4(uint32_t x, uint32_t *out)
{
    if (FMT == GPSIQ_SC08) {
        // a field per byte, then its sign bit spread over the rest of the byte (8 * 0x1e = 0xf0, 2 * 0x7e = 0xfc: inside the byte)
#pragma unroll
        for (int k = 0; k < 8 / BITS; ++k) {
            uint32_t t;
            if (BITS == 4) {
                t = (x >> (16 * k)) & 0xffffu;
                t = (t | (t << 8)) & 0x00ff00ffu;
                t = (t | (t << 4)) & 0x0f0f0f0fu;
                t |= (t & 0x08080808u) * 0x1eu;
            } else {
                t = (x >> (8 * k)) & 0xffu;
                t = (t | (t << 12)) & 0x000f000fu;
                t = (t | (t << 6)) & 0x03030303u;
                t |= (t & 0x02020202u) * 0x7eu;
            }
            out[k] = t;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16 / BITS; ++k)                          // one sample per dword: I below, Q above
            out[k] = ((uint32_t) field_of(x, 2 * BITS * k, BITS) & 0xffffu) | ((uint32_t) field_of(x, 2 * BITS * k + BITS, BITS) << 16);
    }
}

// Arguments as pack_stream's, without the counter.  Writes exactly 2 * nsamp elements per block.
template <int BITS, int FMT>
__global__ __launch_bounds__(kPackThreads) void unpack_stream(const uint8_t *__restrict__ src, size_t src_stride, uint8_t *__restrict__ dst,
                                                               size_t dst_stride, int nsamp, uint32_t units, uint32_t tiles, uint64_t total)
{
    constexpr int DST = unpack_unit_dst_bytes(BITS, FMT), PER = DST / 16;      // dwords a packed dword makes: 2, 4, 4, 8
    constexpr int ELEMS = 128 / BITS;                                          // elements of a unit
    const uint64_t nelem = (uint64_t) 2 * (uint64_t) (uint32_t) nsamp, dst_len = nelem * FMT;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint64_t blk = w / tiles;
        const uint32_t tile = (uint32_t) (w - blk * tiles);
        const uint8_t *bs = src + blk * src_stride;
        uint8_t *bd = dst + blk * dst_stride;
#pragma unroll
        for (int j = 0; j < kPackUnitsPerThread; ++j) {
            const uint64_t u = ((uint64_t) tile * kPackUnitsPerThread + j) * kPackThreads + threadIdx.x;
            if (u >= units) continue;
            if ((u + 1) * DST <= dst_len) {                           // all of the unit is the block's: its 16 packed bytes are too
                const Quad in = load16(bs + u * 16);
                if constexpr (PER == 2) {                           // 4 bit -> int8: two packed dwords fill a store
#pragma unroll
                    for (int k = 0; k < 4; k += 2) {
                        uint32_t a[2], b[2];
                        unpack4<BITS, FMT>(in.w[k], a);
                        unpack4<BITS, FMT>(in.w[k + 1], b);
                        store16(bd + u * DST + (size_t) k * 8, Quad{{a[0], a[1], b[0], b[1]}});
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t o[PER];
                        unpack4<BITS, FMT>(in.w[k], o);
#pragma unroll
                        for (int q = 0; q < PER; q += 4)
                            store16(bd + u * DST + (size_t) (k * PER + q) * 4, Quad{{o[q], o[q + 1], o[q + 2], o[q + 3]}});
                    }
                }
            } else {
                // the ragged end of the block, an element at a time
                for (uint64_t e = u * ELEMS; e < nelem; ++e) {
                    const uint64_t bit = e * BITS;
                    const int v = field_of(bs[bit >> 3], (int) (bit & 7), BITS);
                    if (FMT == GPSIQ_SC16) reinterpret_cast<int16_t *>(bd)[e] = (int16_t) v;
                    else reinterpret_cast<int8_t *>(bd)[e] = (int8_t) v;
                }
            }
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// The kernels that exist, as data: what gpsiq_pack.cpp looks up.  nullptr: no such kernel.
PackFn pack_kernel(int fmt, int bits)
{
    if (fmt == GPSIQ_SC08) return bits == 4 ? pack_stream<GPSIQ_SC08, 4> : bits == 2 ? pack_stream<GPSIQ_SC08, 2> : nullptr;
    if (fmt == GPSIQ_SC16) return bits == 4 ? pack_stream<GPSIQ_SC16, 4> : bits == 2 ? pack_stream<GPSIQ_SC16, 2> : nullptr;
    return nullptr;
}

UnpackFn unpack_kernel(int bits, int fmt)
{
    if (fmt == GPSIQ_SC08) return bits == 4 ? unpack_stream<4, GPSIQ_SC08> : bits == 2 ? unpack_stream<2, GPSIQ_SC08> : nullptr;
    if (fmt == GPSIQ_SC16) return bits == 4 ? unpack_stream<4, GPSIQ_SC16> : bits == 2 ? unpack_stream<2, GPSIQ_SC16> : nullptr;
    return nullptr;
}
}  // namespace gpsiq
