// gpsiq_drift.h -- Drift: the rounding enclosure of GPSIQ_NCO_REFERENCE, which decides a candidate sample from the block's
// start state alone (gpsiq_exact.cpp has the overview; the device's twin without tables is DriftLite in gpsiq_eval.h).
// Host only, header only.
#ifndef GPSIQ_DRIFT_H
#define GPSIQ_DRIFT_H

#include "gpsiq_walk.h"

#include <cmath>

namespace gpsiq {

// The double accumulator at sample n WITHOUT walking it: a rigorous enclosure.
//
// Every addition of the reference loop is the exact sum plus a rounding error e_j, so the unwrapped phase after n samples is
// U_n = x_0 + n*c + d_n with d_n = e_0 + ... + e_{n-1} (wraps are exact; the carrier's y + 1.0 is one more rounding).  While
// state and sum lie in one binade b (ulp u_b) the state is a multiple of u_b and the sum is rounded on that grid, so the
// addition adds S_b = rnd(|c|/u_b)*u_b and e_j = +-(S_b - |c|) =: +-eps_b, a constant of the binade (ties to even: constant
// from the second addition inside the binade on).  Let G be the piecewise linear function on [0, L] with slope eps_b/S_b
// in binade b (0 below the lowest binade counted), continued over the wraps as G^(U) = floor(U/L)*G(L) + G(U mod L).  A steady
// step moves the phase by +-S_b and G^ by +-eps_b = e_j exactly, so the steady steps telescope:
//     d_n = G^(U_n) - G(x_0) + sum over the IRREGULAR steps j of (e_j - [G^(U_{j+1}) - G^(U_j)]),
// and the irregular steps of one cycle are few and each is bounded by the ulp of its binade: the step that enters a binade
// (rounded on the new, coarser grid from a state on the finer one: <= 1.001 u_b; twice that where |c|/u_b ends in exactly one
// half and the first addition from an odd mantissa rounds the other way), the wrap (carrier: the sum in [1, 2) or y + 1.0,
// <= 1.51 u_top; code: an ordinary addition in [512, 1024) followed by an exact subtraction, 0.51 u_top for the piece of G it
// skips) and the handful of additions below 8|c| (G is flat there; <= 3 u of the lowest binade counted).  Since G^ is
// Lipschitz with a constant of ~2^-44, U_n on the right may be replaced by R_n = x_0 + n*c (exact integer arithmetic in
// units of c's ulp) at a cost far below one unit.  The enclosure is ~0.3 % as wide as the a-priori window n * 2^-54 the
// candidates are found with (tests/test_reference_nco_host.py holds it against the walked accumulator on adversarial
// addends: ties, binade-edge starts; observed use of the half-width <= 0.6), so nearly every candidate is decided here, from
// the block's start state alone -- which is what lets the blocks of a timeline be evaluated on any thread, device or
// process once the serial carrier chain has given their start states.
struct Drift {
    typedef __int128 i128;
    bool    valid = false;
    int     kind = 1;
    bool    neg = false;
    double  L = 1.0;
    int64_t ec = 0, mc = 0;           // |c| = mc * 2^(ec - 1075)
    int     b_lo = 0, b_top = 0;      // biased exponents of the binades that count
    double  ulp_c = 0.0;
    double  g[64], Gedge[65];         // slope in binade b_lo + i; G at its lower edge
    double  edge_lo = 0.0;            // lower edge of binade b_lo (G = 0 below)
    double  GL = 0.0, gmax = 0.0, Acyc = 0.0;
    int     cell_shift = 0;           // log2(cell / ulp_c): a cell is 1/512 cycle (carrier) or one chip (code)
    i128    Lint = 0;                 // L / ulp_c

    void setup(double c, int kind_)
    {
        kind = kind_;
        L = kind == 0 ? (double) kCaSeqLen : 1.0;
        const int top_exp = kind == 0 ? 1023 + 9 : 1022;
        neg = c < 0.0;
        const uint64_t bc = bits_of(c) & ~(UINT64_C(1) << 63);
        ec = (int64_t) (bc >> 52);
        mc = (int64_t) ((bc & kMant) | (kMant + 1));
        // the same addends NcoWalk's fast walk takes: at least 2^6 below the top binade, not absurdly small, the code phase only climbs
        valid = !(ec > top_exp - 6 || ec < top_exp - 40 || (kind == 0 && neg));
        if (!valid) return;
        ulp_c = from_bits((uint64_t) (ec - 52) << 52);
        b_lo = (int) ec + 3; b_top = top_exp;
        edge_lo = from_bits((uint64_t) b_lo << 52);
        double G = 0.0, allow = 0.0;
        gmax = 0.0;
        for (int b = b_lo; b <= b_top; ++b) {
            const int s = b - (int) ec;
            int64_t dm = mc >> s;
            const int64_t rem = mc & (((int64_t) 1 << s) - 1), half = (int64_t) 1 << (s - 1);
            bool tie = false;
            if (rem > half) ++dm;
            else if (rem == half) { tie = true; dm += dm & 1; }
            const double delta = (double) ((dm << s) - mc);                  // eps_b / ulp_c, exact
            const double Sb = (double) dm * (double) ((int64_t) 1 << s);     // S_b / ulp_c, exact
            const double gb = delta / Sb;
            const double lo = from_bits((uint64_t) b << 52);
            const double width = (kind == 0 && b == b_top) ? L - lo : lo;    // [512, 1023) for the code phase's top binade
            g[b - b_lo] = gb;
            Gedge[b - b_lo] = G;
            G += gb * width;
            if (std::fabs(gb) > gmax) gmax = std::fabs(gb);
            allow += 1.001 * from_bits((uint64_t) (b - 52) << 52) * (tie ? 2.0 : 1.0);
        }
        Gedge[b_top - b_lo + 1] = G;
        GL = G;
        const double u_top = from_bits((uint64_t) (b_top - 52) << 52), u_lo = from_bits((uint64_t) (b_lo - 52) << 52);
        Acyc = allow + 3.0 * u_lo + (kind == 0 ? 0.51 : 1.51) * u_top;
        cell_shift = kind == 0 ? (int) (1075 - ec) : (int) (1075 - ec - 9);
        Lint = kind == 0 ? (i128) kCaSeqLen << (1075 - ec) : (i128) 1 << (1075 - ec);
    }

    inline double Gof(double x) const            // 0 <= x <= L
    {
        if (x < edge_lo) return 0.0;
        if (x >= L) return GL;
        const int b = (int) (bits_of(x) >> 52);
        return Gedge[b - b_lo] + g[b - b_lo] * (x - from_bits((uint64_t) b << 52));
    }

    // x0 in units of ulp_c, cut below one unit
    inline i128 units(double x0) const
    {
        const uint64_t bx = bits_of(x0);
        const int64_t ex = (int64_t) (bx >> 52);
        if (ex == 0) return 0;
        const i128 mx = (i128) ((bx & kMant) | (kMant + 1));
        const int64_t sh = ex - ec;
        return sh >= 0 ? mx << sh : (sh > -64 ? mx >> -sh : (i128) 0);
    }

    // The enclosure [*lo, *hi], in units of ulp_c, of the double path's phase at sample n, counted from phase 0 of the block's
    // first cycle / code period and unwrapped; false: none (a start outside [0, L), an addend the fast walk does not take).
    bool enclose(double x0, long n, i128 *lo, i128 *hi) const
    {
        if (!valid || !(x0 >= 0.0 && x0 < L)) return false;
        const i128 R = neg ? units(x0) - (i128) n * mc : units(x0) + (i128) n * mc;     // x0 + n*c
        // floor(R / L) and the rest, without a 128-bit division: L = 2^sh (carrier) or 1023 * 2^sh units
        const int sh = (int) (1075 - ec);
        const int64_t hi_part = (int64_t) (R >> sh);                                    // floor(R / 2^sh): cycles, or chips (< 2^40)
        int64_t q;
        if (kind == 1) q = hi_part;
        else { q = hi_part / kCaSeqLen; if (hi_part % kCaSeqLen < 0) --q; }
        const i128 r = R - (i128) q * Lint;
        const double core = (double) q * GL + Gof((double) r * ulp_c) - Gof(x0);
        const double I = ((double) (q < 0 ? -q : q) + 3.0) * Acyc;
        const double eta = 4.0 * gmax * (std::fabs(core) + I) + 1e-12 * (std::fabs(core) + std::fabs((double) q * GL)) + 4.0 * gmax * L * 0x1p-52;
        *lo = R + (i128) std::floor((core - I - eta) / ulp_c) - 2;
        *hi = R + (i128) std::ceil((core + I + eta) / ulp_c) + 2;
        return true;
    }

    // The cell (LUT step or chip, unwrapped like the enclosure) that holds the double path's phase at sample n, when the
    // enclosure lies inside one cell; false: undecided (no enclosure, or a boundary inside it -- also every phase the
    // reference wraps to exactly 1.0).
    bool cell_at(double x0, long n, i128 *cell) const
    {
        i128 lo, hi;
        if (!enclose(x0, n, &lo, &hi)) return false;
        const i128 c0 = lo >> cell_shift, c1 = hi >> cell_shift;                          // arithmetic shifts: floor for negative phases too
        if (c0 != c1) return false;
        *cell = c0;
        return true;
    }
};

}  // namespace gpsiq
#endif
