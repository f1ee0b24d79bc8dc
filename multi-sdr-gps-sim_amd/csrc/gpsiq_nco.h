// gpsiq_nco.h -- Nco: one double accumulator of the reference loop, walked exactly for ANY addend and start state (the general
// walker of GPSIQ_NCO_REFERENCE; gpsiq_exact.cpp has the overview).  Host only, header only.
#ifndef GPSIQ_NCO_H
#define GPSIQ_NCO_H

#include "gpsiq_walk.h"

namespace gpsiq {

// One double accumulator of the reference loop.  kind 0: code phase (wrap at 1023 chips,
// gps.c:2789-2792); kind 1: carrier phase (wrap into [0,1), gps.c:2821-2826).
struct Nco {
    double x, c;      // state used by sample n; the addend
    long   n, wraps;  // wraps: number of wraps on the way to sample n (code: code periods completed)
    int    kind;

    // Per binade of x (indexed by the exponent difference to the addend), filled on first use: the settled step dm in
    // ulps (state 2: not usable -- exact tie, or step zero), and the run length from the binade's entry edge written as
    // span = k*dm + rem, so that a run entered within one step of the edge needs a comparison instead of a division.
    struct Piece { int64_t dm, span, k, rem, kdm; int state; };       // state 0: not built, 1: usable, 2: take the probing path
    Piece piece[55] = {};

    inline double step(double v, int *wrapped) const
    {
        double y = v + c;
        *wrapped = 0;
        if (kind == 0) {
            if (y >= (double) kCaSeqLen) { y -= (double) kCaSeqLen; *wrapped = 1; }
        } else {
            if (y >= 1.0) { y -= 1.0; *wrapped = 1; }
            else if (y < 0.0) { y += 1.0; *wrapped = 1; }
        }
        return y;
    }

    // The last mantissa (53 bits, in ulps) a run of settled steps may reach inside the binade with biased exponent `expo`.
    // Upwards that is the last mantissa of the binade, 2^53 - 1 -- or of the code period: the wrap comes before the binade
    // ends only in the code phase's top binade [512, 1024), 1023 = 1023 * 2^43 ulps there (the carrier's top binade
    // [0.5, 1) ends exactly at its wrap).  Downwards the run must stay strictly above the binade's first value 2^52 ulps: a
    // sum that falls below it is rounded on the finer grid of the binade underneath, so the last step onto (or from) 2^52
    // is a real addition.
    inline int64_t run_end(int64_t expo, bool down) const
    {
        if (down) return ((int64_t) 1 << 52) + 1;
        return (kind == 0 && expo == 1023 + 9 ? (int64_t) kCaSeqLen << 43 : (int64_t) 1 << 53) - 1;
    }

    // Largest j such that x, x + S, ..., x + j*S (S = dm ulps of x's binade) all stay inside x's binade and short of
    // the wrap, capped at `cap`.  mx = x's 53-bit mantissa.
    inline long run_length(int64_t mx, int64_t dm, uint64_t expo, long cap) const
    {
        if (dm > 0) {
            const int64_t j = (run_end((int64_t) expo, false) - mx) / dm;
            return j < cap ? (long) j : cap;
        }
        if (c < 0.0 && mx < run_end((int64_t) expo, true)) return 0;      // on the binade's first value
        if (dm < 0) {
            const int64_t j = (mx - run_end((int64_t) expo, true)) / -dm;
            return j < cap ? (long) j : cap;
        }
        return cap;                                      // the addend is below half an ulp: the phase stands still
    }

    void build_piece(Piece &p, int64_t shift, int64_t ex, int64_t mc, bool neg) const
    {
        // x + c inside x's binade is x + S with S = rnd(c/u) ulps, whatever x is -- unless c/u ends in exactly one
        // half, where the rounding goes to even and depends on x's parity (left to the probing path of advance())
        int64_t dm = shift == 0 ? mc : (shift >= 53 ? 0 : mc >> shift);
        bool tie = false;
        if (shift > 0 && shift <= 53) {
            const int64_t rem = mc & (((int64_t) 1 << shift) - 1), half = (int64_t) 1 << (shift - 1);
            if (rem > half) ++dm;
            else if (rem == half) tie = true;
        }
        p.state = (tie || dm == 0) ? 2 : 1;
        if (p.state == 2) return;
        p.dm = dm;
        // the longest run: from the binade's first mantissa 2^52 up, or from its last one 2^53 - 1 down
        p.span = neg ? (((int64_t) 1 << 53) - 1) - run_end(ex, true) : run_end(ex, false) - ((int64_t) 1 << 52);
        p.k = p.span / dm;
        p.kdm = p.k * dm;
        p.rem = p.span - p.kdm;
    }

    // Move to sample `target` (>= n).
    void advance(long target)
    {
        const uint64_t bc = bits_of(c) & ~(UINT64_C(1) << 63);
        const int64_t ec = (int64_t) (bc >> 52), mc = (int64_t) ((bc & kMant) | (kMant + 1));
        const bool neg = c < 0.0;
        while (n < target) {
            const uint64_t bx = bits_of(x);
            const int64_t ex = (int64_t) (bx >> 52);
            if (ex != 0 && ec != 0 && ex >= ec && ex - ec <= 54) {
                Piece &p = piece[ex - ec];
                if (p.state == 0) build_piece(p, ex - ec, ex, mc, neg);
                if (p.state == 1) {
                    const int64_t mx = (int64_t) ((bx & kMant) | (kMant + 1));
                    // distance of x from the edge the run was measured from; the run is (span - off) / dm steps long
                    const int64_t off = neg ? (((int64_t) 1 << 53) - 1) - mx : mx - ((int64_t) 1 << 52);
                    int64_t run, moved;
                    if (off <= p.rem) { run = p.k; moved = p.kdm; }
                    else if (off <= p.rem + p.dm) { run = p.k - 1; moved = p.kdm - p.dm; }
                    else if (off > p.span) { run = 0; moved = 0; }
                    else { run = (p.span - off) / p.dm; moved = run * p.dm; }
                    const long cap = target - n;
                    if (run >= cap) { run = cap; moved = run * p.dm; }
                    if (run > 0) {
                        x = from_bits((bx & ~kMant) | ((uint64_t) (neg ? mx - moved : mx + moved) & kMant));
                        n += run;
                        if (run == cap) return;
                    }
                    // the next addition leaves the binade or wraps: the reference's own operation
                    int w;
                    const double y = step(x, &w);
                    if (y == x && !w) { n = target; return; }    // e.g. exactly 2^k with a negative addend below a quarter ulp: stuck for good
                    x = y; ++n; wraps += w;
                    continue;
                }
            }
            // zero / subnormal, a binade below the addend's, or the tie case: real additions, and a jump once two
            // consecutive additions inside one binade have shown the settled step
            int wy;
            const double y = step(x, &wy);
            if (y == x && !wy) { n = target; return; }           // the addend no longer moves x: it never will again
            const uint64_t by = bits_of(y);
            if (wy || (bx >> 52) != (by >> 52) || (bx >> 52) == 0) {
                x = y; ++n; wraps += wy;
                continue;
            }
            if (n + 1 == target) { x = y; ++n; return; }
            int wz;
            const double z = step(y, &wz);
            const uint64_t bz = bits_of(z);
            if (wz || (bz >> 52) != (by >> 52)) { x = z; n += 2; wraps += wz; continue; }
            const int64_t my = (int64_t) ((by & kMant) | (kMant + 1)), mz = (int64_t) ((bz & kMant) | (kMant + 1));
            const long run = run_length(my, mz - my, by >> 52, target - (n + 1));    // samples n+1 .. n+1+run are y + j*S
            x = from_bits((by & ~kMant) | ((uint64_t) (my + (int64_t) run * (mz - my)) & kMant));
            n += 1 + run;
        }
    }
};

}  // namespace gpsiq
#endif
