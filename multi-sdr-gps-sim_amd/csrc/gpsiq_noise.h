// gpsiq_noise.h -- receiver noise (include/gpsiq.h, "Receiver noise"), shared by the host (gpsiq_device.cpp: the tables and the
// host twin) and the device (gpsiq_kernels.hip): same source, integer arithmetic only, so both agree bit for bit.
//
// Sample n of absolute block B draws from lane stream l = n & 63, row j = n >> 6 -- the row kernels' own lane/row mapping, so a
// lane of a wave walks its stream one LCG step per row:
//   X_0 = splitmix64(seed ^ splitmix64(B*64 + l)),  X_{j+1} = X_j * kMul + kInc  (PCG32's LCG),  w = xsh_rr(X_j)
//   zI = z(w & 0xffff), zQ = z(w >> 16)
// z() is a 512-segment piecewise-linear inverse normal CDF with an exact 64-point tail (gpsiq_noise_knots.h), scaled to sigma.
// On the device the scaled table is Entry[kEntries]: entries 0..510 are the segments (base S[k], slope S[k+1]-S[k]), entries
// 511..574 the tail points (base S_tail[f], slope 0), so one 8-byte gather per component serves both cases.
//
// The output level stage (include/gpsiq_rows.h, "Output level") follows the noise and lives here with it: level::apply is the
// contract's scale, round and clamp of one component, for the kernels that work sample by sample and as the statement the tile
// body's own copy is held against.
#ifndef GPSIQ_NOISE_H
#define GPSIQ_NOISE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GPSIQ_NOISE_HD __host__ __device__
#else
#define GPSIQ_NOISE_HD
#endif

namespace gpsiq {
namespace noise {

constexpr uint64_t kMul = UINT64_C(0x5851f42d4c957f2d);
constexpr uint64_t kInc = UINT64_C(0x14057b7ef767814f);
constexpr int kEntries = 511 + 64;          // segments 0..510, then the tail points
constexpr int kTabEntries = 576;            // padded: what the device table holds (the last entry is never read)

struct Entry {
    int32_t base;    // S[k] (segment) or S_tail[f] (tail)
    int32_t slope;   // S[k+1] - S[k] >= 0, or 0 in the tail
};

// what a launch needs: the scaled table on the device (nullptr: noise off), the seed, the absolute index of the descriptor
// array's block 0, and max|z| (the int16 plain-add core needs every |I + zI| <= 32767)
// With the output level on (mult != 0) tab is never null: an all-zero table stands in while the noise is off.
struct Launch {
    const Entry *tab = nullptr;
    uint64_t     seed = 0;
    uint64_t     block = 0;
    long         max_z = 0;
    uint32_t     mult = 0;     // output level: Q16 multiplier, 0 = off
    int32_t      qmax = 0;     //               symmetric clamp
};

GPSIQ_NOISE_HD inline uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + UINT64_C(0x9e3779b97f4a7c15);
    z = (z ^ (z >> 30)) * UINT64_C(0xbf58476d1ce4e5b9);
    z = (z ^ (z >> 27)) * UINT64_C(0x94d049bb133111eb);
    return z ^ (z >> 31);
}

// PCG32's output permutation of the state before the step
GPSIQ_NOISE_HD inline uint32_t xsh_rr(uint64_t x)
{
    const uint32_t xs = (uint32_t) (((x >> 18) ^ x) >> 27);
    const uint32_t rot = (uint32_t) (x >> 59);
    return (xs >> rot) | (xs << ((0u - rot) & 31u));
}

// (A, C) with X_j = A*X_0 + C after j steps of X <- X*mul + inc (the usual square-and-multiply jump-ahead)
GPSIQ_NOISE_HD inline void jump(uint64_t j, uint64_t mul, uint64_t inc, uint64_t *A, uint64_t *C)
{
    uint64_t am = 1, ap = 0;
    while (j) {
        if (j & 1u) { am *= mul; ap = ap * mul + inc; }
        inc = (mul + 1u) * inc;
        mul *= mul;
        j >>= 1;
    }
    *A = am;
    *C = ap;
}

// lane stream l of absolute block B, before row 0
GPSIQ_NOISE_HD inline uint64_t lane_start(uint64_t seed, uint64_t block, uint32_t lane)
{
    return splitmix64(seed ^ splitmix64(block * 64u + lane));
}

// one 16-bit draw -> signed noise value, in accumulator units
GPSIQ_NOISE_HD inline int32_t z(const Entry *tab, uint32_t u)
{
    const uint32_t k = (u >> 6) & 511u, f = u & 63u;
    const Entry e = tab[k < 511u ? k : 511u + f];
    const int32_t mag = e.base + ((e.slope * (int32_t) f) >> 6);
    return (u & 0x8000u) ? -mag : mag;
}

// the two components of sample (block, n); host twin and the kernels that work sample by sample
GPSIQ_NOISE_HD inline void sample(const Entry *tab, uint64_t seed, uint64_t block, uint32_t n, int32_t *zi, int32_t *zq)
{
    uint64_t A, C;
    jump(n >> 6, kMul, kInc, &A, &C);
    const uint32_t w = xsh_rr(A * lane_start(seed, block, n & 63u) + C);
    *zi = z(tab, w & 0xffffu);
    *zq = z(tab, w >> 16);
}

}  // namespace noise

namespace level {

// out = clamp(floor((A * mult + 32768) / 65536), -qmax, qmax); |A| < 2^19 and mult < 2^24, so the product needs 64 bits and the
// quotient fits 32 (the shift of a negative int64_t is arithmetic: floor)
GPSIQ_NOISE_HD inline int32_t apply(int32_t A, uint32_t mult, int32_t qmax)
{
    const int32_t y = (int32_t) (((int64_t) A * (int64_t) (int32_t) mult + 32768) >> 16);
    return y < -qmax ? -qmax : y > qmax ? qmax : y;
}

}  // namespace level
}  // namespace gpsiq
#endif
