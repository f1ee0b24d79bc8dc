// gpsiq_exact.cpp — GPSIQ_NCO_REFERENCE: the reference's double-precision NCOs, reproduced exactly.
//
// The reference advances code_phase and carr_phase by sequential double additions
// (gps.c:2789-2792, gps.c:2821-2826).  The library's default model is the closed form on integers of
// include/gpsiq.h; given the same block-start state the two differ in a few samples per 10^7, where a
// phase sits within the double path's accumulated rounding drift of a chip or LUT boundary.  This file
// finds exactly those samples on the host and describes them as patches for the device, and it
// carries carr_phase from block to block as the reference's own accumulator would leave it, so that a
// whole run equals the reference element for element.
//
// How, without stepping 260 000 additions per channel and block:
//   * x += c in double is piecewise linear.  While x stays inside one binade it is a multiple of the
//     binade's ulp u and the addition adds the constant S = rnd(c/u)*u (ties to even: constant from the
//     second addition inside the binade on, when the parity has settled).  Nco::advance() does the
//     reference's own operation (a real double addition, then the wrap rule) at binade crossings and
//     wraps and jumps over the steady run in between with one integer division (S straight from the addend's
//     mantissa; the rare exact-tie binades are probed with two real additions): about a dozen pieces
//     per carrier cycle or code period.
//   * Only samples whose fixed-point phase lies within the drift bound of a boundary can differ:
//     |double path - real arithmetic| <= n * 2^-54 cycle (carrier, values < 1) or n * 2^-44 chip (code,
//     values < 1024), the fixed-point path is within (n/2 + 1) units of its last place of real arithmetic.
//     Those candidates are the n with (a + n*b) mod 2^k inside a narrow window: found with a
//     Euclid-style descent in O(log) per hit (first_in_window), typically none or one per channel and block.
//   * At every candidate the double path's LUT index / chip is decided from the block's START state by a rigorous enclosure of
//     the accumulated rounding (Drift: 99.5+ % of the candidates), else by walking the accumulator (NcoWalk); where (LUT index,
//     sign) differ from the closed form a patch {block, sample, slot, index, sign} is emitted.  The device runs the fixed-point
//     kernels unchanged and then recomputes the patched samples (apply_patches in gpsiq_kernels.hip).
// Only the carrier chain is serial (block k of a channel starts where the double accumulator left block k-1): NcoWalk walks it
// from wrap to wrap through a per-block table of its dozen distinct cycles (built eight cycles at a time where the host has
// AVX-512), and RefWalk runs chains and evaluations as tasks on the shared thread pool, piece by piece, so that devices render
// behind them; gpsiq_reference_chain / gpsiq_reference_seeded export the two halves for sharding over processes.
//
// Where each of these lives:
//   Nco, the general walker                                      gpsiq_nco.h
//   first_in_range, candidates: the candidate search             gpsiq_candidates.h
//   NcoWalk: the wrap-to-wrap table and its AVX-512 build        gpsiq_ncowalk.h (the scalar core, WalkCore: gpsiq_walk.h)
//   Drift, the rounding enclosure                                gpsiq_drift.h
//   CodeCache, nav_bit, and what this file offers other files    gpsiq_exact.h
//   RefWalk, the task scheduler                                  gpsiq_refwalk.cpp (declared in gpsiq_internal.h)
//   eval_block, chain_block, reference_timeline, the C exports   here
#include "gpsiq_exact.h"
#include "gpsiq_candidates.h"
#include "gpsiq_drift.h"
#include "gpsiq_ncowalk.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace gpsiq {

static_assert(kCaSeqLen == GPSIQ_CA_SEQ_LEN, "gpsiq_walk.h");

// process-wide counts (gpsiq_reference_stats): candidates seen, decided from the start state alone, walked (carrier / code)
static std::atomic<uint64_t> g_stats[4];

double chain_block(double f_carr, double delt, int nsamp, double start)
{
    NcoWalk cw;
    cw.setup(f_carr * delt, 1);
    return cw.run(start, nsamp);
}

// The parallel half: one channel of one block, given the double the reference's accumulator holds at its start (1.0 included,
// see below).  Quantises the descriptor seeded from it (-> q) and appends the samples where the double path takes another LUT
// entry or sign than the closed form.  The candidates are found without visiting samples (candidates()); each is decided by
// the drift enclosure from the block's start state, and only where a boundary lies inside the enclosure are the accumulators
// walked (from the block's start, to the last undecided sample).
// slot_of: the block's descriptors up to this channel (blk[0 .. i]), or null with `slot` given: the device order counts the
// active channels before this one (gpsiq_set_descriptors), which is only looked up when a patch is written.
// seed_override: the fixed-point carrier phase the descriptor is seeded with instead of the one cut from `start` (the device
// renders from an ESTIMATE of the start state and learns the true one later, gpsiq_evaldev.cpp): the closed form then runs
// |seed - fixed(start)| units beside the one seeded from the truth, the candidate window is that much wider, and the patches are
// what the double path from the TRUE start takes against that closed form.
int eval_block(const gpsiq_chan_t &ch, double start, double delt, int nsamp, int block, int slot,
               CodeCache *codes, gpsiq_qchan_t *qq, std::vector<gpsiq_patch_t> *out, bool no_drift,
               const gpsiq_chan_t *blk, int i_in_blk, const uint64_t *seed_override)
{
    // a start of exactly 1.0 (a wrap of the block before that rounded up to one) is phase 0 of the closed form (mod 1); the
    // reference goes on from 1.0, and sample 0, where it indexes its table at 512, is patched.  The start state replaces the
    // descriptor's own carr_phase (handed to the quantiser as the carried phase: the 296-byte descriptor is not copied)
    if (!(start >= 0.0 && start <= 1.0)) return fail(GPSIQ_E_RANGE, "prn %d: start phase %g outside [0, 1]", ch.prn, start);
    const uint64_t seeded_true = carr_phase_to_fixed(start == 1.0 ? 0.0 : start);
    const uint64_t seeded = seed_override ? (*seed_override & ((UINT64_C(1) << GPSIQ_CARR_FRAC_BITS) - 1)) : seeded_true;
    uint64_t seed_off = (seeded_true - seeded) & ((UINT64_C(1) << GPSIQ_CARR_FRAC_BITS) - 1);       // |difference| mod 2^59
    if (seed_off > (UINT64_C(1) << (GPSIQ_CARR_FRAC_BITS - 1))) seed_off = (UINT64_C(1) << GPSIQ_CARR_FRAC_BITS) - seed_off;
    int qrc;
    if (ch.carr_phase >= 0.0 && ch.carr_phase < 1.0) qrc = quantize_one(ch, delt, nsamp, &seeded, qq, nullptr);
    else {                         // the descriptor's own phase is the 1.0 the reference handed back (or garbage): not the quantiser's business here
        gpsiq_chan_t tmp = ch;
        tmp.carr_phase = 0.0;
        qrc = quantize_one(tmp, delt, nsamp, &seeded, qq, nullptr);
    }
    if (qrc != GPSIQ_OK) return qrc;
    const gpsiq_qchan_t &q = *qq;
    const long ns = nsamp;
    if (ns <= 0) return GPSIQ_OK;
    const double carr_inc = ch.f_carr * delt, code_inc = ch.f_code * delt;
    // drift bounds at the end of the block, in units of the fixed-point formats (see the header)
    const uint64_t w_carr = ((uint64_t) ns << (GPSIQ_CARR_FRAC_BITS - 54)) + (uint64_t) ns / 2 + 4 + seed_off;
    const uint64_t w_code = ((uint64_t) ns << (GPSIQ_CODE_FRAC_BITS - 44)) + (uint64_t) ns / 2 + 4;
    // scratch that keeps its capacity from block to block (an evaluation task runs thousands of these back to back)
    static thread_local std::vector<long> t_carr, t_code, open_c, open_k;
    static thread_local std::vector<double> xc, xk;
    static thread_local std::vector<long> periods;
    t_carr.clear(); t_code.clear(); open_c.clear(); open_k.clear();
    constexpr size_t kCap = 256;
    bool every = false;
    if (carr_inc != 0.0 || seed_off != 0)          // a zero addend leaves both paths constant, and equal when seeded alike
        every |= !candidates(q.carr_phase, (uint64_t) q.carr_step, GPSIQ_CARR_FRAC_BITS - 9, w_carr, ns, kCap, &t_carr);
    every |= !candidates(q.code_frac, q.code_step, GPSIQ_CODE_FRAC_BITS, w_code, ns, kCap, &t_code);
    if (every) {                  // too many to list (a sample rate far outside the format's design range): every sample, both accumulators
        t_carr.resize((size_t) ns);
        for (long n = 0; n < ns; ++n) t_carr[(size_t) n] = n;
        t_code = t_carr;
    }
    if (t_carr.empty() && t_code.empty()) return GPSIQ_OK;
    // A sample that is no candidate of an accumulator has that accumulator's closed-form index by construction: the carrier is
    // looked at in the carrier's candidates only, the code phase in the code's.
    // 1. decide from the start state alone: cells[k] >= 0 the double path's cell, -1 undecided (walk)
    static thread_local std::vector<long> cell_c, cell_k;
    cell_c.assign(t_carr.size(), -1); cell_k.assign(t_code.size(), -1);
    const double x0c = start;                                                   // 1.0 included: undecided by construction, walked
    if (!every && !no_drift) {
        Drift::i128 cell;
        if (!t_carr.empty()) {
            Drift dc;
            dc.setup(carr_inc, 1);
            for (size_t k = 0; k < t_carr.size(); ++k)
                if (dc.cell_at(x0c, t_carr[k], &cell)) cell_c[k] = (long) (cell & 511);
                else open_c.push_back(t_carr[k]);
        }
        if (!t_code.empty()) {
            Drift dk;
            dk.setup(code_inc, 0);
            for (size_t k = 0; k < t_code.size(); ++k)
                if (dk.cell_at(ch.code_phase, t_code[k], &cell)) cell_k[k] = (long) cell;
                else open_k.push_back(t_code[k]);
        }
    } else {
        open_c = t_carr;
        open_k = t_code;
    }
    // 2. walk what is left (from the block's start: the walk reports the state at its targets on the way)
    if (!open_c.empty()) {
        NcoWalk cw;
        cw.setup(carr_inc, 1);
        xc.resize(open_c.size());
        (void) cw.run(start, open_c.back() + 1, open_c.data(), (int) open_c.size(), xc.data());
    }
    if (!open_k.empty()) {
        NcoWalk kw;
        kw.setup(code_inc, 0);
        xk.resize(open_k.size()); periods.resize(open_k.size());
        (void) kw.run(ch.code_phase, open_k.back() + 1, open_k.data(), (int) open_k.size(), xk.data(), periods.data());
    }
    g_stats[0].fetch_add(t_carr.size() + t_code.size(), std::memory_order_relaxed);
    g_stats[1].fetch_add(t_carr.size() + t_code.size() - open_c.size() - open_k.size(), std::memory_order_relaxed);
    g_stats[2].fetch_add(open_c.size(), std::memory_order_relaxed);
    g_stats[3].fetch_add(open_k.size(), std::memory_order_relaxed);
    const uint8_t *ca = codes->get(ch.prn);
    size_t ic = 0, ik = 0, jc = 0, jk = 0;                     // merge of the two ascending candidate lists
    while (ic < t_carr.size() || ik < t_code.size()) {
        const long n = ik >= t_code.size() || (ic < t_carr.size() && t_carr[ic] <= t_code[ik]) ? t_carr[ic] : t_code[ik];
        const bool in_c = ic < t_carr.size() && t_carr[ic] == n, in_k = ik < t_code.size() && t_code[ik] == n;
        // fixed-point path (include/gpsiq.h)
        const uint64_t P = (q.carr_phase + (uint64_t) q.carr_step * (uint64_t) n) & ((UINT64_C(1) << GPSIQ_CARR_FRAC_BITS) - 1);
        const unsigned idx_f = (unsigned) (P >> (GPSIQ_CARR_FRAC_BITS - 9));
        const u128 T = (u128) q.code_frac + (u128) q.code_step * (uint64_t) n;
        const uint64_t A = (uint64_t) q.chip0 + (uint64_t) (T >> GPSIQ_CODE_FRAC_BITS);
        const unsigned chip_f = (unsigned) (A % GPSIQ_CA_SEQ_LEN);
        const long per_f = (long) (A / GPSIQ_CA_SEQ_LEN);
        const unsigned neg_f = ca[chip_f] ^ nav_bit(ch, ((long) ch.icode + per_f) / 20);
        // double path
        unsigned idx = idx_f;
        if (in_c) {
            if (cell_c[ic] >= 0) idx = (unsigned) cell_c[ic];
            else {
                idx = (unsigned) (int) std::floor(xc[jc++] * 512.0);                      // gps.c:2775
                if (idx > 511u) idx = 511u;   // carr_phase == 1.0 (a negative phase within 2^-54 of zero): the reference indexes past its table there
            }
            ++ic;
        }
        unsigned neg_d = neg_f;
        if (in_k) {
            unsigned chip_d;
            long per_d;
            if (cell_k[ik] >= 0) { chip_d = (unsigned) (cell_k[ik] % GPSIQ_CA_SEQ_LEN); per_d = cell_k[ik] / GPSIQ_CA_SEQ_LEN; }
            else { chip_d = (unsigned) (int) xk[jk]; per_d = periods[jk]; ++jk; }         // gps.c:2817, 2791-2793
            neg_d = ca[chip_d] ^ nav_bit(ch, ((long) ch.icode + per_d) / 20);             // gps.c:2791-2811
            ++ik;
        }
        if (idx != idx_f || neg_d != neg_f) {
            if (blk) { slot = 0; for (int j = 0; j < i_in_blk; ++j) slot += blk[j].prn > 0; blk = nullptr; }
            gpsiq_patch_t p;
            p.block = (uint32_t) block; p.sample = (uint32_t) n;
            p.slot = (uint8_t) slot; p.neg = (uint8_t) neg_d; p.lut = (uint16_t) idx;
            out->push_back(p);
        }
    }
    return GPSIQ_OK;
}

double chain_block_true(double f_carr, double delt, int nsamp, double start) { return chain_block(f_carr, delt, nsamp, start); }

// GPSIQ_CHAIN_VERIFY=N (read per call): every N-th block linked through its certified map is also walked serially from the same
// start state and must end on the same double; 0 / unset: off
int chain_verify_every()
{
    const char *e = std::getenv("GPSIQ_CHAIN_VERIFY");
    const int n = e ? std::atoi(e) : 0;
    return n > 0 ? n : 0;
}

// one channel of one block for the device path (gpsiq_evaldev.cpp): the (block, channel) pairs its enclosure cannot decide
int eval_block_host(const gpsiq_chan_t &ch, double start, const uint64_t *seed, double delt, int nsamp, int block, int slot, gpsiq_qchan_t *q,
                    std::vector<gpsiq_patch_t> *out)
{
    CodeCache codes;
    return eval_block(ch, start, delt, nsamp, block, slot, &codes, q, out, false, nullptr, 0, seed);
}

// the piece ends of a timeline cut every `chunk` blocks (RefWalk adds the last one, nblocks)
static std::vector<int> even_ends(int nblocks, int chunk)
{
    std::vector<int> ends;
    for (int b = chunk; b < nblocks; b += chunk) ends.push_back(b);
    return ends;
}

// the walker's end state into the caller's arrays (either may be null)
static void end_state(const RefWalk &w, int nchan, double *carr_end, int *last_prn)
{
    for (int i = 0; i < nchan; ++i) {
        if (carr_end) carr_end[i] = w.carr_end[i];
        if (last_prn) last_prn[i] = w.last_prn[i];
    }
}

int reference_timeline(const gpsiq_chan_t *ch, int nblocks, int nchan, double delt, int nsamp,
                       gpsiq_qchan_t *q, std::vector<gpsiq_patch_t> *patches, double *carr_end, int *last_prn,
                       const double *carr_in, const int *prn_in)
{
    if (nblocks == 1) {
        // the drop-in block call (one 0.1 s block per call, ~100 us all told): chain and evaluation of the sixteen channels right
        // here, without the scheduler's mutexes, condition variables and task state
        CodeCache codes;
        patches->clear();
        int slot = 0;
        for (int i = 0; i < nchan; ++i) {
            const gpsiq_chan_t &d = ch[i];
            if (d.prn <= 0) {
                (void) quantize_one(d, delt, nsamp, nullptr, &q[i], nullptr);
                if (carr_end) carr_end[i] = 0.0;
                if (last_prn) last_prn[i] = 0;
                continue;
            }
            const double start = carr_in && prn_in && prn_in[i] == d.prn ? carr_in[i] : d.carr_phase;
            if (!(start >= 0.0 && start <= 1.0) || !(std::fabs(d.f_carr * delt) < 0.5))
                return fail(GPSIQ_E_RANGE, "block 0: carrier phase or Doppler outside the NCO format");
            const int erc = eval_block(d, start, delt, nsamp, 0, slot++, &codes, &q[i], patches, std::getenv("GPSIQ_NO_DRIFT") != nullptr);
            if (erc != GPSIQ_OK) { char msg[300]; std::snprintf(msg, sizeof msg, "%s", gpsiq_last_error()); return fail(erc, "block 0: %.280s", msg); }
            if (carr_end) carr_end[i] = chain_block(d.f_carr, delt, nsamp, start);
            if (last_prn) last_prn[i] = d.prn;
        }
        std::sort(patches->begin(), patches->end(), patch_before);
        return GPSIQ_OK;
    }
    // a handful of pieces so that a thread-starved host still overlaps chains and evaluations; a short timeline is one piece
    RefWalk w(ch, nblocks, nchan, delt, nsamp, q, carr_in, prn_in, even_ends(nblocks, nblocks > 64 ? (nblocks + 15) / 16 : nblocks));
    w.run();
    if (w.rc != GPSIQ_OK) return fail(w.rc, "%s", w.err);
    w.all_patches(patches);
    end_state(w, nchan, carr_end, last_prn);
    return GPSIQ_OK;
}

}  // namespace gpsiq

using namespace gpsiq;

// the patches into the caller's buffer, or how many there were when it has no room for them
static int give_patches(const std::vector<gpsiq_patch_t> &v, gpsiq_patch_t *patches, int max_patches, int *npatches)
{
    *npatches = (int) v.size();
    if (v.size() > (size_t) max_patches) return fail(GPSIQ_E_RANGE, "%zu patches, room for %d", v.size(), max_patches);
    if (!v.empty()) std::memcpy(patches, v.data(), v.size() * sizeof(gpsiq_patch_t));
    return GPSIQ_OK;
}

extern "C" int gpsiq_reference_chain(const gpsiq_chain_in_t *in, int nblocks, int nchan, double fs, int nsamp,
                                     const double *carr_in, const int32_t *prn_in, double *carr_start, double *carr_end, int32_t *last_prn)
{
    if ((!in || !carr_start) && nblocks) return fail(GPSIQ_E_ARG, "null pointer");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    if (nsamp < 0 || !(fs > 0.0) || (!carr_in != !prn_in)) return fail(GPSIQ_E_ARG, "bad nsamp %d / fs %g / continuation state", nsamp, fs);
    // one task per channel when there is a thread for every channel; else pieces, so that the channels share the threads evenly
    const int chunk = host_threads() >= nchan || nblocks <= 64 ? nblocks : (nblocks + 7) / 8;
    RefWalk w(nullptr, nblocks, nchan, 1.0 / fs, nsamp, nullptr, carr_in, prn_in, even_ends(nblocks, chunk));
    w.in = in; w.chain_only = true; w.start_out = carr_start;
    w.run();
    if (w.rc != GPSIQ_OK) return fail(w.rc, "%s", w.err);
    end_state(w, nchan, carr_end, last_prn);
    return GPSIQ_OK;
}

extern "C" int gpsiq_reference_seeded(const gpsiq_chan_t *ch, int nblocks, int nchan, double fs, int nsamp, const double *carr_start,
                                      gpsiq_qchan_t *q, gpsiq_patch_t *patches, int max_patches, int *npatches)
{
    if ((!ch || !q || !carr_start) && nblocks) return fail(GPSIQ_E_ARG, "null pointer");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    if (nsamp < 0 || !(fs > 0.0) || max_patches < 0 || !npatches || (max_patches && !patches))
        return fail(GPSIQ_E_ARG, "bad nsamp %d / fs %g / patch buffer", nsamp, fs);
    for (size_t k = 0; k < (size_t) nblocks * (size_t) nchan; ++k)
        if (ch[k].prn > 0 && !(carr_start[k] >= 0.0 && carr_start[k] <= 1.0)) return fail(GPSIQ_E_RANGE, "start phase %zu outside [0, 1]", k);
    RefWalk w(ch, nblocks, nchan, 1.0 / fs, nsamp, q, nullptr, nullptr, even_ends(nblocks, nblocks > 64 ? (nblocks + 15) / 16 : nblocks));
    w.seeds = carr_start;
    w.run();
    if (w.rc != GPSIQ_OK) return fail(w.rc, "%s", w.err);
    std::vector<gpsiq_patch_t> v;
    w.all_patches(&v);
    return give_patches(v, patches, max_patches, npatches);
}

extern "C" void gpsiq_reference_stats(uint64_t out[4])
{
    if (!out) return;
    for (int k = 0; k < 4; ++k) out[k] = g_stats[k].load(std::memory_order_relaxed);
}

extern "C" void gpsiq_chain_inputs(const gpsiq_chan_t *ch, int n, gpsiq_chain_in_t *out)
{
    if (!ch || !out) return;
    for (int k = 0; k < n; ++k) { out[k].f_carr = ch[k].f_carr; out[k].carr_phase = ch[k].carr_phase; out[k].prn = ch[k].prn; out[k].reserved = 0; }
}

extern "C" int gpsiq_reference_batch(const gpsiq_chan_t *ch, int nblocks, int nchan, double fs, int nsamp,
                                     gpsiq_qchan_t *q, gpsiq_patch_t *patches, int max_patches, int *npatches,
                                     double *carr_phase_out)
{
    if ((!ch || !q) && nblocks) return fail(GPSIQ_E_ARG, "null descriptor pointer");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    if (nsamp < 0 || !(fs > 0.0) || max_patches < 0 || !npatches || (max_patches && !patches))
        return fail(GPSIQ_E_ARG, "bad nsamp %d / fs %g / patch buffer", nsamp, fs);
    std::vector<gpsiq_patch_t> v;
    int rc = reference_timeline(ch, nblocks, nchan, 1.0 / fs, nsamp, q, &v, carr_phase_out, nullptr, nullptr, nullptr);
    if (rc) return rc;
    return give_patches(v, patches, max_patches, npatches);
}
