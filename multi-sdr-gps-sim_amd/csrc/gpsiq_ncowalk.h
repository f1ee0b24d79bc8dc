// gpsiq_ncowalk.h -- NcoWalk: the reference's double accumulators walked from wrap to wrap (WalkCore, gpsiq_walk.h) through a
// per-block table of whole cycles, which is built eight cycles at a time where the host has AVX-512 (gpsiq_exact.cpp has the
// overview).  Host only, header only.  GPSIQ_WALK_BUCKETS and GPSIQ_WALK_KLOW are compile-time knobs of this header: a
// program that sets either must not link an object that holds NcoWalk as well (scripts/ubench_walk.cpp).
#ifndef GPSIQ_NCOWALK_H
#define GPSIQ_NCOWALK_H

#include "gpsiq_nco.h"

#include <cmath>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace gpsiq {

// The accumulators walked from wrap to wrap.
//
// Nco::advance costs a dozen dependent pieces per carrier cycle / code period, ~70 ns.  For the common case (a normal
// addend well below the accumulator's range, no exact-tie binade) NcoWalk has the same walk in a leaner form -- between
// two wraps the phase climbs (or, with a negative carrier addend, descends) through the binades from the addend's own to
// the top one; the lowest three hold 1, 2, 4 steps: plain additions there cost less than a table piece each (five binades
// measured 5 % slower on the GPU box's host, scripts/ubench_walk.cpp); above them one piece per binade, with the run length from a per-binade table -- and, on top of it, a map from wrap to wrap.
// Right after a wrap the state is a multiple of U = the ulp of the binade the wrap is taken in (carrier: 2^-52 for
// y - 1.0 with y in [1, 2), 2^-53 for y + 1.0 in [0.5, 1); code: 2^-43 for y - 1023.0 with y in [512, 1024)).  Start the
// same cycle from x0 + d*U instead of x0: as long as every RESULT of the cycle's additions stays inside the binade it had
// (and on its side of the wrap limit), every rounding drops the same bits -- d*U is a multiple of every ulp involved, an
// even one wherever a tie could occur, since addends with an exact-tie binade above the plain additions take the general
// walker -- and the whole cycle is the first one translated: same number of samples, final state moved by d*U.  The cycle
// walk therefore also returns the range of d for which that holds (the distance of every result to the edges of its
// binade, two units short on either side because a sum that crosses an edge is rounded on the other grid), and the cycle
// becomes an entry {first state, last state, state increment, samples} of a small table.  As the start state sweeps the
// addend's width every binade edge on the way is crossed one step earlier exactly once, so the table has about as many
// entries as a cycle has binades (a dozen or two); a block of 260 000 samples at 2.6 kHz Doppler is 260 carrier cycles, of
// which the first ~17 are walked and the rest are look-ups on integers.  The one rounding that is not translation
// invariant is the wrap itself when it is an exact tie (the kept bit's parity moves with d): such a cycle is never tabled.
// The addends change with every block (gps.c:2042-2043), so a table lives for one block.
struct NcoWalk : WalkCore<64> {

#if defined(__x86_64__)
    // ---- eight carrier cycles walked at once (AVX-512) -------------------------------------------------------------------
    // A walked cycle is ~10 dependent binade steps, and a block needs a dozen of them before its wrap-to-wrap table is
    // complete.  Discovered one at a time as the chain reaches them they are a third of the chain's time; but a cycle depends
    // only on its start state, every lane goes through the same binades in the same order, and the per-binade piece
    // (step, run length) is the same for all of them: eight start states take the vector form of climb<true> / descend<true>
    // -- the same additions, the same slack notes, lane for lane -- in about the time of one.  Anything that is not the plain
    // case in some lane (a run that needs the division, a state of exactly 1.0, a tie on the wrap, a lane that leaves the
    // binade sequence) marks that lane not-ok; such a start state is walked by the scalar code when the chain gets there.
    struct Batch { int64_t m[8], lo[8], hi[8], m2[8], steps[8]; bool ok[8]; };

#define GPSIQ_AVX512 __attribute__((target("avx512f,avx512dq")))
#define GPSIQ_NOTE(v, act)                                                                                               \
    do {                                                                                                                 \
        const __m512i b_ = _mm512_castpd_si512(v);                                                                       \
        const __m512i e_ = _mm512_srli_epi64(b_, 52);                                                                    \
        const __m512i sh_ = _mm512_sub_epi64(uexp_v, e_);                                                                \
        const __mmask8 bad_ = _mm512_cmplt_epi64_mask(sh_, zero) | _mm512_cmpgt_epi64_mask(sh_, sixty2) | _mm512_cmpeq_epi64_mask(e_, zero); \
        okm &= (__mmask8) ~(bad_ & (act));                                                                               \
        const __m512i mx_ = _mm512_or_si512(_mm512_and_si512(b_, mant), one52);                                          \
        const __m512i l_ = _mm512_sub_epi64(two, _mm512_srlv_epi64(_mm512_sub_epi64(mx_, one52), sh_));                  \
        const __m512i h_ = _mm512_sub_epi64(_mm512_srlv_epi64(_mm512_sub_epi64(one53, mx_), sh_), two);                  \
        lo = _mm512_mask_max_epi64(lo, (act), lo, l_);                                                                   \
        hi = _mm512_mask_min_epi64(hi, (act), hi, h_);                                                                   \
    } while (0)

    // One table binade for all lanes (run + the addition that leaves it): x in binade ec + s on entry.  kDown: negative addend.
    // Returns with x = the last value inside the binade (after the run), n advanced by the run; the caller adds c.
    template <bool kDown>
    GPSIQ_AVX512 inline void batch_level(int s, __m512d &x, __m512i &n, __m512i &lo, __m512i &hi, __mmask8 &okm, const __m512i uexp_v) const
    {
        const __m512i zero = _mm512_setzero_si512(), two = _mm512_set1_epi64(2), sixty2 = _mm512_set1_epi64(62);
        const __m512i mant = _mm512_set1_epi64((int64_t) kMant), one52 = _mm512_set1_epi64((int64_t) 1 << 52), one53 = _mm512_set1_epi64((int64_t) 1 << 53);
        const Piece &p = T[s];
        const __m512d cv = _mm512_set1_pd(c);
        __m512i b = _mm512_castpd_si512(x);
        okm &= _mm512_cmpeq_epi64_mask(_mm512_srli_epi64(b, 52), _mm512_set1_epi64(ec + s));          // still on the common path
        __m512i mx = _mm512_or_si512(_mm512_and_si512(b, mant), one52);
        if (p.tie) {                                                   // an odd mantissa in a tie binade: one real addition first
            const __mmask8 odd = _mm512_test_epi64_mask(mx, _mm512_set1_epi64(1));
            if (odd) {
                x = _mm512_mask_add_pd(x, odd, x, cv);
                n = _mm512_mask_add_epi64(n, odd, n, _mm512_set1_epi64(1));
                GPSIQ_NOTE(x, odd);
                b = _mm512_castpd_si512(x);
                okm &= _mm512_cmpeq_epi64_mask(_mm512_srli_epi64(b, 52), _mm512_set1_epi64(ec + s));
                mx = _mm512_or_si512(_mm512_and_si512(b, mant), one52);
            }
        }
        const __m512i off = kDown ? _mm512_sub_epi64(_mm512_set1_epi64(((int64_t) 1 << 53) - 1), mx) : _mm512_sub_epi64(mx, one52);
        const __mmask8 c1 = _mm512_cmple_epi64_mask(off, _mm512_set1_epi64(p.rem));
        const __mmask8 c2 = (__mmask8) (~c1 & _mm512_cmple_epi64_mask(off, _mm512_set1_epi64(p.rem + p.dm)));
        const __mmask8 c3 = _mm512_cmpgt_epi64_mask(off, _mm512_set1_epi64(p.span));
        okm &= (__mmask8) (c1 | c2 | c3);                              // the run that needs a division: scalar code
        __m512i run = _mm512_maskz_mov_epi64(c1, _mm512_set1_epi64(p.k));
        run = _mm512_mask_mov_epi64(run, c2, _mm512_set1_epi64(p.k - 1));
        __m512i moved = _mm512_maskz_mov_epi64(c1, _mm512_set1_epi64(p.kdm));
        moved = _mm512_mask_mov_epi64(moved, c2, _mm512_set1_epi64(p.kdm - p.dm));
        const __m512i mx2 = kDown ? _mm512_sub_epi64(mx, moved) : _mm512_add_epi64(mx, moved);
        x = _mm512_castsi512_pd(_mm512_or_si512(_mm512_andnot_si512(mant, b), _mm512_and_si512(mx2, mant)));
        n = _mm512_add_epi64(n, run);
        const __mmask8 ran = _mm512_cmpgt_epi64_mask(run, zero);
        GPSIQ_NOTE(x, ran);
    }

#define GPSIQ_VCONSTS(UEXP)                                                                                               \
    const __m512i zero = _mm512_setzero_si512(), two = _mm512_set1_epi64(2), sixty2 = _mm512_set1_epi64(62);              \
    const __m512i mant = _mm512_set1_epi64((int64_t) kMant), one52 = _mm512_set1_epi64((int64_t) 1 << 52), one53 = _mm512_set1_epi64((int64_t) 1 << 53); \
    const __m512i uexp_v = _mm512_set1_epi64(UEXP);                                                                       \
    const __m512d cv = _mm512_set1_pd(c), thr_v = _mm512_set1_pd(thr), one = _mm512_set1_pd(1.0);                         \
    (void) zero; (void) two; (void) sixty2; (void) mant; (void) one52; (void) one53; (void) uexp_v; (void) cv; (void) thr_v; (void) one

    // positive addend, the binades below the table: plain additions (at most 2^(kLow + 1) + 1 of them)
    GPSIQ_AVX512 inline void batch_low_up(__m512d &x, __m512i &n, __m512i &lo, __m512i &hi, __mmask8 &okm) const
    {
        GPSIQ_VCONSTS(1023);
        for (int it = 0; it < (2 << kLow) + 2; ++it) {
            const __mmask8 act = _mm512_cmp_pd_mask(x, thr_v, _CMP_LT_OQ);
            if (!act) break;
            x = _mm512_mask_add_pd(x, act, x, cv);
            n = _mm512_mask_add_epi64(n, act, n, _mm512_set1_epi64(1));
            GPSIQ_NOTE(x, act);
        }
        okm &= (__mmask8) ~_mm512_cmp_pd_mask(x, thr_v, _CMP_LT_OQ);
    }

    // positive addend, table binade ec + s: the run and the addition that leaves it.  true: that was the wrap (s == top), x is
    // the state after it
    GPSIQ_AVX512 inline bool batch_level_up(int s, int top, __m512d &x, __m512i &n, __m512i &lo, __m512i &hi, __mmask8 &okm) const
    {
        GPSIQ_VCONSTS(1023);
        batch_level<false>(s, x, n, lo, hi, okm, uexp_v);
        const __m512d y = _mm512_add_pd(x, cv);                        // leaves the binade; at the top: wraps
        n = _mm512_add_epi64(n, _mm512_set1_epi64(1));
        if (s < top) { x = y; GPSIQ_NOTE(x, (__mmask8) 0xff); return false; }
        okm &= _mm512_cmp_pd_mask(y, one, _CMP_GE_OQ);
        GPSIQ_NOTE(y, (__mmask8) 0xff);
        const __m512d bb = _mm512_sub_pd(y, x);
        const __m512d err = _mm512_add_pd(_mm512_sub_pd(x, _mm512_sub_pd(y, bb)), _mm512_sub_pd(cv, bb));    // the rounding error of x + c, exactly
        okm &= (__mmask8) ~_mm512_cmp_pd_mask(_mm512_abs_pd(err), _mm512_set1_pd(0x1p-53), _CMP_EQ_OQ);      // a tie on the grid the wrap is taken on
        x = _mm512_sub_pd(y, one);
        return true;
    }

    // negative addend, table binade ec + s: the run and the addition into the binade underneath
    GPSIQ_AVX512 inline void batch_level_down(int s, __m512d &x, __m512i &n, __m512i &lo, __m512i &hi, __mmask8 &okm) const
    {
        GPSIQ_VCONSTS(1022);
        batch_level<true>(s, x, n, lo, hi, okm, uexp_v);
        x = _mm512_add_pd(x, cv);
        n = _mm512_add_epi64(n, _mm512_set1_epi64(1));
        GPSIQ_NOTE(x, (__mmask8) 0xff);
    }

    // negative addend, below the table: plain additions until the sum turns negative, then + 1.0; x: the state after the wrap
    GPSIQ_AVX512 inline void batch_tail_down(__m512d &x, __m512i &n, __m512i &lo, __m512i &hi, __mmask8 &okm) const
    {
        GPSIQ_VCONSTS(1022);
        const __m512d zd = _mm512_setzero_pd();
        okm &= _mm512_cmp_pd_mask(x, thr_v, _CMP_LT_OQ);
        const __m512d c2 = _mm512_mul_pd(cv, _mm512_set1_pd(-2.0));
        __mmask8 open = 0xff;
        __m512d r_end = zd;
        for (int it = 0; it < (4 << kLow) + 4 && open; ++it) {
            const __m512d y = _mm512_add_pd(x, cv);
            n = _mm512_mask_add_epi64(n, open, n, _mm512_set1_epi64(1));
            const __mmask8 ng = (__mmask8) (open & _mm512_cmp_pd_mask(y, zd, _CMP_LT_OQ)), ps = (__mmask8) (open & ~ng);
            if (ng) {
                const __m512d r = _mm512_add_pd(y, one);
                // y's own rounding: exact when x lies in the addend's binade (only its sign has to hold), else noted
                const __mmask8 same = (__mmask8) (ng & _mm512_cmpeq_epi64_mask(_mm512_srli_epi64(_mm512_castpd_si512(x), 52), _mm512_set1_epi64(ec)));
                const __m512i h = _mm512_sub_epi64(_mm512_cvttpd_epi64(_mm512_mul_pd(_mm512_sub_pd(zd, y), _mm512_set1_pd(0x1p53))), two);
                hi = _mm512_mask_min_epi64(hi, same, hi, h);
                const __m512d ny = _mm512_sub_pd(zd, y);
                GPSIQ_NOTE(ny, (__mmask8) (ng & ~same));
                const __m512d bb = _mm512_sub_pd(r, y);
                const __m512d err = _mm512_add_pd(_mm512_sub_pd(y, _mm512_sub_pd(r, bb)), _mm512_sub_pd(one, bb));
                const __mmask8 badr = (__mmask8) (_mm512_cmp_pd_mask(r, one, _CMP_GE_OQ) | _mm512_cmp_pd_mask(_mm512_abs_pd(err), _mm512_set1_pd(0x1p-54), _CMP_EQ_OQ));
                okm &= (__mmask8) ~(badr & ng);
                GPSIQ_NOTE(r, (__mmask8) (ng & ~badr));
                r_end = _mm512_mask_mov_pd(r_end, ng, r);
                open &= (__mmask8) ~ng;
            }
            if (ps) {
                // x <= 2|c|: x + c is exact (Sterbenz) for this x and every translated one; it only has to stay non-negative
                const __mmask8 st = (__mmask8) (ps & _mm512_cmp_pd_mask(x, c2, _CMP_LE_OQ));
                const __m512i l = _mm512_sub_epi64(two, _mm512_cvttpd_epi64(_mm512_mul_pd(y, _mm512_set1_pd(0x1p53))));
                lo = _mm512_mask_max_epi64(lo, st, lo, l);
                GPSIQ_NOTE(y, (__mmask8) (ps & ~st));
                x = _mm512_mask_mov_pd(x, ps, y);
            }
        }
        okm &= (__mmask8) ~open;
        x = r_end;
    }

    // positive addend: climb<true> for eight post-wrap states m (units of 2^-52)
    GPSIQ_AVX512 void walk8_up(int64_t m_max, Batch *io) const
    {
        const __m512i m = _mm512_loadu_si512(io->m);
        __m512d x = _mm512_mul_pd(_mm512_cvtepi64_pd(m), _mm512_set1_pd(0x1p-52));
        __m512i n = _mm512_setzero_si512(), lo = _mm512_sub_epi64(_mm512_setzero_si512(), m), hi = _mm512_sub_epi64(_mm512_set1_epi64(m_max), m);
        __mmask8 okm = 0xff;
        batch_low_up(x, n, lo, hi, okm);
        const int top = (int) (top_exp - ec);
        for (int s = kLow + 1; s <= top; ++s)
            if (batch_level_up(s, top, x, n, lo, hi, okm)) break;
        okm &= _mm512_cmp_pd_mask(x, _mm512_set1_pd(1.0), _CMP_LT_OQ);
        const __m512i m2 = _mm512_cvttpd_epi64(_mm512_mul_pd(x, _mm512_set1_pd(0x1p52)));
        _mm512_storeu_si512(io->lo, lo); _mm512_storeu_si512(io->hi, hi); _mm512_storeu_si512(io->m2, m2); _mm512_storeu_si512(io->steps, n);
        for (int q = 0; q < 8; ++q) io->ok[q] = (okm >> q) & 1;
    }

    // negative addend: descend<true> for eight post-wrap states m (units of 2^-53)
    GPSIQ_AVX512 void walk8_down(int64_t m_max, Batch *io) const
    {
        const __m512i m = _mm512_loadu_si512(io->m);
        __m512d x = _mm512_mul_pd(_mm512_cvtepi64_pd(m), _mm512_set1_pd(0x1p-53));
        __m512i n = _mm512_setzero_si512(), lo = _mm512_sub_epi64(_mm512_setzero_si512(), m), hi = _mm512_sub_epi64(_mm512_set1_epi64(m_max), m);
        __mmask8 okm = (__mmask8) (0xff & _mm512_cmp_pd_mask(x, _mm512_set1_pd(1.0), _CMP_LT_OQ));        // a state of exactly 1.0: scalar code
        const int top = (int) (top_exp - ec);
        for (int s = top; s > kLow; --s) batch_level_down(s, x, n, lo, hi, okm);
        batch_tail_down(x, n, lo, hi, okm);
        const __m512i m2 = _mm512_cvttpd_epi64(_mm512_mul_pd(x, _mm512_set1_pd(0x1p53)));
        _mm512_storeu_si512(io->lo, lo); _mm512_storeu_si512(io->hi, hi); _mm512_storeu_si512(io->m2, m2); _mm512_storeu_si512(io->steps, n);
        for (int q = 0; q < 8; ++q) io->ok[q] = (okm >> q) & 1;
    }
    // the buckets [k0, k1] of one entry, eight per store
    GPSIQ_AVX512 static void fill8(int64_t *inc, uint64_t *tag, int64_t k0, int64_t k1, int64_t vinc, uint64_t vtag)
    {
        const __m512i vi = _mm512_set1_epi64(vinc), vt = _mm512_set1_epi64((int64_t) vtag);
        int64_t k = k0;
        for (; k + 7 <= k1; k += 8) { _mm512_storeu_si512(inc + k, vi); _mm512_storeu_si512(tag + k, vt); }
        for (; k <= k1; ++k) { inc[k] = vinc; tag[k] = vtag; }
    }
#undef GPSIQ_NOTE
#undef GPSIQ_VCONSTS
    static bool wide() { static const bool w = __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("avx512f"); return w; }
#endif   // __x86_64__

    // the state at sample `target` (>= n) of a walk that is at sample n in state x; counts the wraps on the way
    inline double state_at(double x, long n, long target, long *wraps) const
    {
        while (n < target && cycle(x, n, target)) ++*wraps;
        return x;
    }

    // wrap-to-wrap table.  Entries are valid each on its own (overlaps are harmless) and are found through 1024 buckets
    // over the range of post-wrap states: a bucket wholly inside an entry carries its increment and sample count (one shift,
    // one load and an add per cycle, no search: the states are as good as random, a binary search would mispredict at every
    // level); the few buckets that straddle an edge fall back to a scan of the entries.
    struct Entry { int64_t first, last, inc; long steps; };
#ifndef GPSIQ_WALK_BUCKETS
#define GPSIQ_WALK_BUCKETS 1024
#endif
    static constexpr int kMaxEntries = 64, kBuckets = GPSIQ_WALK_BUCKETS;     // scripts/ubench_walk.cpp A/Bs the bucket count
    // The buckets live per thread and are never cleared: a bucket belongs to the table of the run (= block) whose stamp it
    // carries (clearing 1024 of them per block cost as much as a hundred look-ups).  Increment and sample count sit in two
    // arrays, so that the chain state -> shift -> load -> add that every cycle waits for is those three instructions and
    // nothing else; stamp and count are read beside it.
    struct Buckets {
        int64_t  inc[kBuckets];
        uint64_t tag[kBuckets];              // (stamp << 32) | samples of the cycle
        uint32_t stamp = 0;
        Buckets() { for (int i = 0; i < kBuckets; ++i) tag[i] = 0; }
        uint32_t next_stamp()
        {
            if (++stamp == 0) { for (int i = 0; i < kBuckets; ++i) tag[i] = 0; stamp = 1; }
            return stamp;
        }
    };

    // A function of its own (and not inlined): in the middle of run() the compiler keeps the state in memory, and the store
    // forwarding on it would cost more than the look-up itself.  rel = state - base.
    __attribute__((noinline)) static void hits(const Buckets *bk, uint32_t stamp, int64_t W, int bshift, long limit,
                                               int64_t *rel_io, long *n_io, long *wraps_io)
    {
        uint64_t rel = (uint64_t) *rel_io;
        long n = *n_io, wraps = *wraps_io;
        for (;;) {
            if (rel >= (uint64_t) W) break;
            const uint64_t idx = rel >> bshift, tag = bk->tag[idx];
            const long steps = (long) (uint32_t) tag;
            if ((uint32_t) (tag >> 32) != stamp || n + steps > limit) break;
            rel += (uint64_t) bk->inc[idx]; n += steps; ++wraps;
        }
        *rel_io = (int64_t) rel; *n_io = n; *wraps_io = wraps;
    }

    // The table of one block: its entries, and the geometry of the post-wrap states they are found by.  A state is counted in
    // units of the grid it lies on right after a wrap, m = x * scale.
    struct WrapTable {
        Entry    tab[kMaxEntries];
        int      ntab = 0;
        long     min_steps;                  // shortest cycle seen
        int      uexp;                       // biased exponent of the binade whose ulp is the state grid
        double   scale, unit;                // 2^(1075 - uexp) and its inverse
        int64_t  m_max;                      // the largest state of the accumulator's range
        int64_t  W, base;                    // post-wrap states: [0, c] (positive addend) or [1 + c, 1) (negative), W units wide from base
        int      bshift = 0;                 // the bucket of state m is (m - base) >> bshift
        Buckets *bk;                         // the thread's buckets; this table's carry `stamp`
        uint32_t stamp;

        WrapTable(const NcoWalk &w, long ns, Buckets *buckets) : min_steps(ns), bk(buckets)
        {
            uexp = w.kind == 0 ? 1023 + 9 : w.neg ? 1022 : 1023;
            scale = from_bits((uint64_t) (1023 + 1075 - uexp) << 52); unit = from_bits((uint64_t) (1023 + uexp - 1075) << 52);
            m_max = w.kind == 0 ? ((int64_t) kCaSeqLen << 43) - 1 : w.neg ? ((int64_t) 1 << 53) - 1 : ((int64_t) 1 << 52) - 1;
            W = (int64_t) (std::fabs(w.c) * scale) + 4;
            base = w.neg ? ((int64_t) 1 << 53) - W : 0;
            while ((W >> bshift) >= kBuckets) ++bshift;
            stamp = bk->next_stamp();
        }

        // an entry for the cycle walked from state ms to state m2 in ne samples, valid for start states ms + [elo, ehi]
        void add(int64_t ms, int64_t m2, long ne, int64_t elo, int64_t ehi)
        {
            Entry &t = tab[ntab++];
            t.first = ms + elo; t.last = ms + ehi; t.inc = m2 - ms; t.steps = ne;
            if (ne < min_steps) min_steps = ne;
            // buckets wholly inside [first, last]
            const int64_t f = t.first - base, l = t.last - base;
            int64_t k0 = f <= 0 ? 0 : ((f - 1) >> bshift) + 1;        // first bucket starting at or after `first`
            int64_t k1 = l >= W ? kBuckets - 1 : ((l + 1) >> bshift) - 1;  // last bucket ending at or before `last`
            if (k1 > kBuckets - 1) k1 = kBuckets - 1;
            if (ne <= 0xffffffffL) {
                const uint64_t tag = ((uint64_t) stamp << 32) | (uint64_t) ne;
#if defined(__x86_64__)
                if (wide()) { fill8(bk->inc, bk->tag, k0, k1, t.inc, tag); return; }
#endif
                for (int64_t k = k0; k <= k1; ++k) { bk->inc[k] = t.inc; bk->tag[k] = tag; }
            }
        }

        // the entry that holds state m (a scan: for the few states whose bucket straddles an edge); null: none
        const Entry *find(int64_t m) const
        {
            for (int i = 0; i < ntab; ++i)
                if (tab[i].first <= m && m <= tab[i].last) return &tab[i];
            return nullptr;
        }
    };

#if defined(__x86_64__)
    // ---- the table built ahead of the chain, eight cycles at a time (walk8_up / walk8_down) ------------------------------
    // one round: the lanes that are new, valid entries
    void take(WrapTable &t, Batch &bt) const
    {
        if (neg) walk8_down(t.m_max, &bt); else walk8_up(t.m_max, &bt);
        for (int q = 0; q < 8 && t.ntab < kMaxEntries; ++q) {
            if (!(bt.ok[q] && bt.lo[q] <= 0 && bt.hi[q] >= 0 && bt.m2[q] >= 0 && bt.m2[q] <= t.m_max && bt.steps[q] > 0)) continue;
            // (not new: a lane that repeats a start state, or fell into an entry already there)
            if (!t.find(bt.m[q])) t.add(bt.m[q], bt.m2[q], (long) bt.steps[q], bt.lo[q], bt.hi[q]);
        }
    }

    // The start states of the next round, from the gaps the entries leave in [d_lo, d_hi]: lanes by gap width (a gap's first
    // uncovered state, and states spread over its inside when it gets more than one lane: an entry reaches down from its start
    // state as well as up).  false: covered but for slivers.
    static bool gap_starts(const WrapTable &t, int64_t d_lo, int64_t d_hi, int64_t m[8])
    {
        int order[kMaxEntries];
        for (int i = 0; i < t.ntab; ++i) {                     // insertion sort by `first`
            int j = i;
            for (; j > 0 && t.tab[order[j - 1]].first > t.tab[i].first; --j) order[j] = order[j - 1];
            order[j] = i;
        }
        int64_t gs[kMaxEntries + 1], gl[kMaxEntries + 1];
        int ng = 0;
        int64_t at = d_lo, open = 0;
        for (int i = 0; i < t.ntab; ++i) {
            const Entry &e = t.tab[order[i]];
            if (e.first > at) { gs[ng] = at; gl[ng] = e.first - at; open += gl[ng]; ++ng; }
            if (e.last + 1 > at) at = e.last + 1;
        }
        if (at <= d_hi) { gs[ng] = at; gl[ng] = d_hi - at + 1; open += gl[ng]; ++ng; }
        if (ng == 0 || open * 64 < (d_hi - d_lo)) return false;
        int q = 0;
        while (q < 8) {
            int w = -1;
            for (int g = 0; g < ng; ++g) if (gl[g] > 0 && (w < 0 || gl[g] > gl[w])) w = g;
            if (w < 0) break;
            int k = (int) ((8 * gl[w] + open / 2) / open);
            if (k < 1) k = 1;
            if (k > 8 - q) k = 8 - q;
            for (int i = 0; i < k; ++i) m[q++] = gs[w] + (gl[w] * i) / k;
            gl[w] = 0;
        }
        for (; q < 8; ++q) m[q] = m[0];                        // fewer gaps than lanes: repeats (dropped as duplicates)
        return true;
    }

    // The post-wrap states of a block fill their range [base, base + W) evenly (a rotation by an irrational step), so with
    // enough cycles in the block every entry will be needed -- and which start states to walk is known without the chain: first
    // eight states spread over the range, then the first uncovered state of every gap those eight entries leave, then once
    // more.  What is still uncovered after that (slivers; cycles that are not the plain case) is found on demand by run(), as
    // before.
    void prefill(WrapTable &t) const
    {
        const int64_t d_lo = t.base < 0 ? 0 : t.base, d_hi = t.base + t.W - 1 > t.m_max ? t.m_max : t.base + t.W - 1;      // the range, inside the accumulator's
        const double range = (double) (d_hi - d_lo);
        Batch bt;
        // Where the entries of the table this thread built last lay, if that was for nearly the same addend (a thread walks the
        // blocks of one channel one after the other; the Doppler moves by a fraction of a hertz per block, and the entries with
        // it): one lane per entry, two rounds, no search.  Else: eight states spread over the range, then twice the gaps the
        // entries leave.
        struct Hint { double c; int n; double at[16]; };
        static thread_local Hint hint = {0.0, 0, {}};
        if (hint.n >= 6 && (hint.c < 0.0) == neg && std::fabs(c - hint.c) <= std::fabs(c) * 0x1p-10) {
            for (int r0 = 0; r0 < hint.n; r0 += 8) {
                for (int q = 0; q < 8; ++q) bt.m[q] = d_lo + (int64_t) (range * hint.at[r0 + q < hint.n ? r0 + q : r0]);
                take(t, bt);
            }
        } else {
            for (int q = 0; q < 8; ++q) bt.m[q] = d_lo + ((d_hi - d_lo) * (2 * q + 1)) / 16;
            for (int round = 0; round < 3 && t.ntab <= kMaxEntries - 8; ++round) {
                take(t, bt);
                if (!gap_starts(t, d_lo, d_hi, bt.m)) break;
            }
        }
        // for the next block of this thread: the middle of every entry, as a fraction of the range
        hint.n = t.ntab < 16 ? t.ntab : 16;
        hint.c = c;
        const double inv = 1.0 / range;
        for (int i = 0; i < hint.n; ++i) {
            const int64_t lo_i = t.tab[i].first < d_lo ? d_lo : t.tab[i].first, hi_i = t.tab[i].last > d_hi ? d_hi : t.tab[i].last;
            hint.at[i] = ((double) (lo_i - d_lo) + (double) (hi_i - lo_i) * 0.5) * inv;
        }
    }
#endif   // __x86_64__

    // The state after ns samples from x0.  targets[nt] (ascending, < ns): samples whose state is wanted as well -> xs[nt]
    // and, if wraps_at is given, the number of wraps before each (code: code periods completed, gps.c:2791-2793).
    double run(double x0, long ns, const long *targets = nullptr, int nt = 0, double *xs = nullptr, long *wraps_at = nullptr) const
    {
        int tk = 0;
        if (ns <= 0) return x0;
        if (general || !(x0 >= 0.0 && x0 < wrap)) {
            Nco a = {x0, c, 0, 0, kind};
            for (; tk < nt; ++tk) { a.advance(targets[tk]); xs[tk] = a.x; if (wraps_at) wraps_at[tk] = a.wraps; }
            a.advance(ns);
            return a.x;
        }
        double x = x0;
        long n = 0, wraps = 0;
        // the targets that lie in [n, upto), from a walk that is at sample n in state x (not disturbed)
        auto visit = [&](double xv, long nv, long upto) {
            long w = wraps;
            for (; tk < nt && targets[tk] < upto; ++tk) {      // each from the one before: a block whose every sample is a target stays linear
                xv = state_at(xv, nv, targets[tk], &w);
                nv = targets[tk];
                xs[tk] = xv;
                if (wraps_at) wraps_at[tk] = w;
            }
        };
        // few cycles in the block: the table would never be read
        if (!(std::fabs(c) * (double) ns > 24.0 * wrap)) {
            visit(x, n, ns);
            while (n < ns && cycle(x, n, ns)) {}
            return x;
        }
        {   // to the first wrap
            const double xs0 = x; const long n0 = n;
            const bool wrapped = cycle(x, n, ns);
            visit(xs0, n0, wrapped ? n : ns + 1);
            if (!wrapped || n == ns) return x;
            ++wraps;
        }
        static thread_local Buckets bkt;
        WrapTable t(*this, ns, &bkt);
        int64_t m = (int64_t) (x * t.scale);                          // exact: the state is a multiple of the unit
#if defined(__x86_64__)
        if (wide() && kind == 1 && std::fabs(c) * (double) ns > 64.0 * wrap) prefill(t);
#endif
        for (;;) {
            // the common case, cycle after cycle: the state's bucket lies wholly inside one entry and names its increment.
            // Stops before a cycle that would pass the end of the block or hold the next target.
            int64_t rel = m - t.base;
            hits(t.bk, t.stamp, t.W, t.bshift, tk < nt && targets[tk] < ns ? targets[tk] : ns, &rel, &n, &wraps);
            m = rel + t.base;
            if (n >= ns) return (double) m * t.unit;
            // a bucket that straddles an edge, a target inside the cycle, the block's end
            const bool inside = rel >= 0 && rel < t.W;
            if (const Entry *e = inside ? t.find(m) : nullptr) {
                if (e->steps > ns - n) break;                         // the block ends inside this cycle
                if (tk < nt && targets[tk] < n + e->steps) visit((double) m * t.unit, n, n + e->steps);
                m += e->inc; n += e->steps; ++wraps;
                continue;
            }
            // not in the table (or 1.0, outside its domain): walk the cycle, noting how far the start state may move
            x = (double) m * t.unit;
            const double xc = x; const long nc = n;
            const bool memo = inside && t.ntab < kMaxEntries && (t.ntab == 0 || ns - n >= 2 * t.min_steps);
            if (!memo) {
                const bool wrapped = cycle(x, n, ns);
                visit(xc, nc, wrapped ? n : ns + 1);
                if (!wrapped) return x;
                ++wraps;
                m = (int64_t) (x * t.scale);
                continue;
            }
            Slack sl = {-m, t.m_max - m, t.uexp, true};               // the start state itself stays inside the accumulator's range
            long ne = 0;
            const bool wrapped = neg ? descend<true>(x, ne, ns - n, &sl) : climb<true>(x, ne, ns - n, &sl);
            n += ne;
            visit(xc, nc, wrapped ? n : ns + 1);
            if (!wrapped) return x;                                   // the block ended inside this cycle
            ++wraps;
            const int64_t m2 = (int64_t) (x * t.scale);
            if (sl.ok && sl.lo <= 0 && sl.hi >= 0 && x < wrap && m2 <= t.m_max) t.add(m, m2, ne, sl.lo, sl.hi);
            m = m2;
        }
        // the last, partial cycle
        x = (double) m * t.unit;
        visit(x, n, ns);
        while (n < ns && cycle(x, n, ns)) {}
        return x;
    }
};

}  // namespace gpsiq
#endif
