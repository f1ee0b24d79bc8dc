// gpsiq_candidates.h -- the candidate search of GPSIQ_NCO_REFERENCE: the samples n of a block whose fixed-point phase
// (a + n*b) mod 2^k lies within the drift bound of a chip or LUT boundary, found without visiting samples (a Euclid-style
// descent, O(log) per hit; gpsiq_exact.cpp has the overview).  Host only, header only.
#ifndef GPSIQ_CANDIDATES_H
#define GPSIQ_CANDIDATES_H

#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace gpsiq {

typedef unsigned __int128 u128;

// Smallest x in [0, bound) with L <= (A*x mod M) <= R, for 0 <= L <= R < M and 0 <= A < M; kNone if there is none.
// The bound goes down the descent with the problem (x < bound needs y <= (A*(bound-1) - L) / M wraps of M), so a search
// that cannot succeed inside the block stops after ~log2(bound) levels instead of ~log(M).
constexpr u128 kNone = ~(u128) 0;
inline u128 first_in_range(uint64_t A, uint64_t M, uint64_t L, uint64_t R, u128 bound)
{
    if (bound == 0) return kNone;
    if (L == 0) return 0;
    if (A == 0) return kNone;
    if (A > M - A) {                 // 2A > M: count downwards instead
        A = M - A;
        const uint64_t l = M - R, r = M - L;
        L = l; R = r;
    }
    const uint64_t lq = L / A, lr = L - lq * A;                   // one division serves the first multiple and L mod A
    const uint64_t k = lq + (lr != 0);
    if ((u128) k * A <= R) return k < bound ? (u128) k : kNone;
    // no multiple of A inside [L, R]: after y wraps of M the window is at M*y + [L, R]; it holds a
    // multiple of A iff ((-M mod A) * y) mod A lies in [L mod A, R mod A]
    const u128 reach = (u128) A * (bound - 1);                    // A * x for the largest x allowed
    if (reach < L) return kNone;
    // the wraps that can matter, a little generously (a double quotient instead of a 128-bit division; the result is checked)
    const u128 ybound = (u128) ((double) (reach - L) / (double) M * (1.0 + 0x1p-40)) + 2;
    const uint64_t mr = M % A;
    // no multiple of A lies in [L, R] here (k * A > R and lr != 0): L and R have the same quotient, so R mod A needs no division
    const u128 y = first_in_range(mr ? A - mr : 0, A, lr, lr + (R - L), ybound);
    if (y == kNone) return kNone;
    const u128 x = ((u128) M * y + L + A - 1) / A;
    return x < bound ? x : kNone;
}

// All n in [0, nsamp) with (a + n*b) mod 2^k within w of 0 (either side), ascending; false if there
// are more than `cap` (the caller then looks at every sample).
inline bool candidates(uint64_t a, uint64_t b, int k, uint64_t w, long nsamp, size_t cap, std::vector<long> *out)
{
    const uint64_t M = UINT64_C(1) << k, mask = M - 1;
    if (2 * w + 1 >= M) return false;
    const uint64_t W = 2 * w + 1;                    // shifted by w the window is [0, W)
    b &= mask;
    long base = 0;
    while (base < nsamp) {
        const uint64_t cur = (uint64_t) (((u128) a + w + (u128) b * (uint64_t) base) & mask);
        long hit;
        if (cur < W) hit = base;
        else {
            const u128 x = first_in_range(b, M, M - cur, M - cur + W - 1, (u128) (nsamp - base));
            if (x == kNone) break;
            hit = base + (long) x;
        }
        if (out->size() >= cap) return false;
        out->push_back(hit);
        base = hit + 1;
    }
    return true;
}

}  // namespace gpsiq
#endif
