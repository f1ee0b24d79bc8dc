// gpsiq_refwalk.cpp -- RefWalk (declared in gpsiq_internal.h): the host side of GPSIQ_NCO_REFERENCE as tasks on the shared
// thread pool, consumed piece by piece while it runs.  What a task computes is gpsiq_exact.cpp's: chain_block, eval_block.
#include "gpsiq_exact.h"
#include "gpsiq_walk.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace gpsiq {

// ---- the host side of GPSIQ_NCO_REFERENCE as tasks ---------------------------------------------------------------
// Only the carrier chain is serial: block b of a channel starts where the double accumulator left block b-1 (gps.c:2821
// carries chan[i].carr_phase; allocateChannel re-initialises it when the slot gets another satellite, gps.c:2208-2214).
// Everything else a block needs -- the quantised descriptor seeded from its start state, the samples where the double path
// leaves the closed form (eval_block) -- depends on that start state alone.  So the timeline is cut into pieces and the work
// into 2 * nchan tasks per piece: CHAIN(i, k) carries channel i through piece k and publishes the start state of each of its
// blocks (after CHAIN(i, k-1)); EVAL(i, k) quantises and patches channel i's blocks of piece k (after CHAIN(i, k), on any
// thread).  The threads of the shared pool (never more than GPSIQ_THREADS allows) take the runnable task of the LOWEST
// piece, chain before evaluation: with a thread per channel every thread alternates between its chain and its evaluations,
// with fewer the timeline is worked through piece-major -- all channels through piece k before anyone starts piece k+1 -- so
// whoever renders (the calling thread of a batch, the device queues of a multi-device batch: they wait for a piece to be
// complete in all channels) still gets its pieces in order and early, and a thread that finds nothing at the front runs a
// chain ahead.  With the start states given (RefWalk::seeds: another process or device walked the chain) only the
// evaluations run; with chain_only only the chains (gpsiq_reference_chain).
RefWalk::RefWalk(const gpsiq_chan_t *ch_, int nblocks_, int nchan_, double delt_, int nsamp_, gpsiq_qchan_t *q_,
                 const double *carr_in_, const int *prn_in_, const std::vector<int> &piece_ends)
    : ch(ch_), nblocks(nblocks_), nchan(nchan_), nsamp(nsamp_), delt(delt_), q(q_), ends(piece_ends), have_in(carr_in_ && prn_in_)
{
    if (ends.empty() || ends.back() != nblocks) ends.push_back(nblocks);
    for (int i = 0; i < GPSIQ_MAX_CHAN; ++i) {
        carr_in[i] = have_in && i < nchan ? carr_in_[i] : 0.0;
        prn_in[i] = have_in && i < nchan ? prn_in_[i] : 0;
        carr_end[i] = 0.0; last_prn[i] = 0;
        chain_next[i] = 0; chain_busy[i] = false; eval_next[i] = 0;
        carr[i] = carr_in[i]; prev[i] = prn_in[i];
    }
    patches.resize((size_t) nchan * ends.size());
    done.reset(new std::atomic<int>[ends.size()]);
    for (size_t k = 0; k < ends.size(); ++k) done[k].store(0, std::memory_order_relaxed);
    pthread_mutex_init(&mu, nullptr);
    pthread_cond_init(&cv, nullptr);
    pthread_cond_init(&task_cv, nullptr);
}

RefWalk::~RefWalk()
{
    pthread_mutex_destroy(&mu);
    pthread_cond_destroy(&cv);
    pthread_cond_destroy(&task_cv);
}

void RefWalk::set_error(int code, const char *text, int block)
{
    pthread_mutex_lock(&mu);
    if (rc == GPSIQ_OK) { rc = code; std::snprintf(err, sizeof err, "block %d: %.280s", block, text); }
    pthread_mutex_unlock(&mu);
    abort_flag.store(true, std::memory_order_release);       // the tasks still to come finish at once (their pieces complete, waiters wake)
}

// channel i through piece k: the start state of every block, then the accumulator after it.  With the blocks' certified maps
// at hand (maps: level 1 of the time-parallel chain, gpsiq_lane.h, walked on the device) a block is one exact subtraction,
// range check and addition (chain_step_mapped) and only the rare block whose map does not apply is walked.
void RefWalk::chain_task(int i, size_t k)
{
    const int b0 = k ? ends[k - 1] : 0, b1 = ends[k];
    double c = carr[i];
    int pv = prev[i];
    long walked = 0, linked = 0;
    for (int b = b0; b < b1; ++b) {
        const size_t at = (size_t) b * nchan + i;
        // a channel's descriptors lie nchan * 296 bytes apart: every block is a cache miss unless it is asked for early
        if (b + 6 < b1) {
            if (in) __builtin_prefetch(&in[at + (size_t) 6 * nchan]); else __builtin_prefetch(&ch[at + (size_t) 6 * nchan]);
            if (maps) chain_prefetch_map(maps, at + (size_t) 6 * nchan);
        }
        const double f_carr = in ? in[at].f_carr : ch[at].f_carr, phase0 = in ? in[at].carr_phase : ch[at].carr_phase;
        const int prn = in ? in[at].prn : ch[at].prn;
        if (prn <= 0) { pv = 0; c = 0.0; start_out[at] = 0.0; continue; }
        if ((b == 0 && !have_in) || pv != prn) c = phase0;
        pv = prn;
        start_out[at] = c;
        if (abort_flag.load(std::memory_order_acquire)) continue;
        // what quantize_one checks of the carrier (the evaluation reports the rest): an addend the walk is defined for
        const double inc = f_carr * delt;
        if (!(c >= 0.0 && c <= 1.0) || !(std::fabs(inc) < 0.5)) {
            set_error(GPSIQ_E_RANGE, "carrier phase or Doppler outside the NCO format", b);
            continue;
        }
        double y;
        if (maps && chain_step_mapped(maps, at, c, &y)) {
            // GPSIQ_CHAIN_VERIFY=N: every N-th block that went through its map is also walked from the same start state
            if (verify_every > 0 && (b + i) % verify_every == 0) {
                const double yw = chain_block(f_carr, delt, nsamp, c);
                if (bits_of(yw) != bits_of(y)) {
                    char msg[160];
                    std::snprintf(msg, sizeof msg, "slot %d: the certified map ends on %.17g, the serial walk on %.17g", i, y, yw);
                    set_error(GPSIQ_E_VERIFY, msg, b);
                }
            }
            c = y; ++linked;
        } else { c = chain_block(f_carr, delt, nsamp, c); ++walked; }
    }
    carr[i] = c; prev[i] = pv;
    if (maps) chain_count(linked, walked);
}

// channel i's blocks of piece k: descriptors and patches from their start states
void RefWalk::eval_task(int i, size_t k, CodeCache *codes)
{
    const int b0 = k ? ends[k - 1] : 0, b1 = ends[k];
    // the task's own list: two evaluations of one channel may run at the same time (pieces k and k+1 on two threads), and
    // whoever takes piece k's patches does so after done[k] has counted this task (release / acquire)
    std::vector<gpsiq_patch_t> *mine = &patches[(size_t) i * ends.size() + k];
    for (int b = b0; b < b1; ++b) {
        const size_t at = (size_t) b * nchan + i;
        if (b + 3 < b1) {                                        // the next descriptors of this channel (five cache lines each, all misses)
            const char *nx = reinterpret_cast<const char *>(&ch[at + (size_t) 3 * nchan]);
            __builtin_prefetch(nx); __builtin_prefetch(nx + 64); __builtin_prefetch(nx + 128); __builtin_prefetch(nx + 192); __builtin_prefetch(nx + 256);
        }
        const gpsiq_chan_t &d = ch[at];
        if (d.prn <= 0 || abort_flag.load(std::memory_order_acquire)) {
            gpsiq_chan_t none = d;
            none.prn = 0;
            (void) quantize_one(none, delt, nsamp, nullptr, &q[at], nullptr);           // an unused slot: zeroes
            continue;
        }
        const int erc = eval_block(d, start[at], delt, nsamp, b, 0, codes, &q[at], mine, no_drift, &ch[(size_t) b * nchan], i);
        if (erc != GPSIQ_OK) set_error(erc, gpsiq_last_error(), b);
    }
}

// the maps of blocks [0, upto) have arrived (the device walks level 1 of a long timeline in two launches): their chain tasks may run
void RefWalk::release_maps(int upto)
{
    pthread_mutex_lock(&mu);
    maps_upto.store(upto, std::memory_order_release);
    pthread_cond_broadcast(&task_cv);
    pthread_mutex_unlock(&mu);
}

void RefWalk::finish_piece(size_t k)
{
    if (done[k].fetch_add(1, std::memory_order_acq_rel) + 1 == nchan) {
        pthread_mutex_lock(&mu);
        pthread_cond_broadcast(&cv);
        pthread_mutex_unlock(&mu);
    }
}

// one thread of the job: take tasks until none is left
void RefWalk::work()
{
    CodeCache codes;
    const size_t np = ends.size();
    pthread_mutex_lock(&mu);
    for (;;) {
        // the runnable task of the lowest piece; chain before evaluation, then the lower channel
        int best_i = -1;
        size_t best_k = np;
        bool best_chain = false, pending = false;
        for (int i = 0; i < nchan; ++i) {
            if (!seeds && chain_next[i] < np) {
                pending = true;
                if (!chain_busy[i] && ends[chain_next[i]] <= maps_upto.load(std::memory_order_acquire) && (chain_next[i] < best_k || (chain_next[i] == best_k && !best_chain))) { best_i = i; best_k = chain_next[i]; best_chain = true; }
            }
            if (!chain_only && eval_next[i] < np) {
                pending = true;
                const size_t ready = seeds ? np : chain_next[i];                      // pieces whose start states are known
                if (eval_next[i] < ready && eval_next[i] < best_k) { best_i = i; best_k = eval_next[i]; best_chain = false; }
            }
        }
        if (best_i < 0) {
            if (!pending) { pthread_cond_broadcast(&task_cv); break; }                // everything is taken: the sleepers may leave too
            pthread_cond_wait(&task_cv, &mu);                                         // a chain in flight will make more runnable
            continue;
        }
        const int i = best_i;
        const size_t k = best_k;
        if (best_chain) chain_busy[i] = true; else ++eval_next[i];
        pthread_mutex_unlock(&mu);
        if (best_chain) {
            chain_task(i, k);
            if (chain_only) finish_piece(k);
            pthread_mutex_lock(&mu);
            chain_busy[i] = false;
            ++chain_next[i];
            // EVAL(i, k) and CHAIN(i, k+1) are runnable now: this thread takes one of them, one sleeper the other (a thread only
            // sleeps after it has found nothing runnable under the lock, and tasks only become runnable here: nothing is missed,
            // and nobody is woken to find nothing -- with 16 threads and tasks of ~50 us a broadcast is most of the work)
            pthread_cond_signal(&task_cv);
        } else {
            eval_task(i, k, &codes);
            finish_piece(k);
            pthread_mutex_lock(&mu);
        }
    }
    pthread_mutex_unlock(&mu);
}

void RefWalk::run()
{
    const size_t total = (size_t) nblocks * (size_t) nchan;
    if (seeds) start = seeds;
    else if (!start_out) { own_start.assign(total ? total : 1, 0.0); start_out = own_start.data(); }
    if (!seeds) start = start_out;
    size_t k0 = 0;
    while (k0 < ends.size() && ends[k0] == 0) ++k0;                                   // empty pieces in front
    for (int i = 0; i < nchan; ++i) { chain_next[i] = k0; eval_next[i] = k0; }
    for (size_t k = 0; k < k0; ++k) done[k].store(nchan, std::memory_order_release);
    if (k0) { pthread_mutex_lock(&mu); pthread_cond_broadcast(&cv); pthread_mutex_unlock(&mu); }
    // a block or two (the drop-in block call): 16 channels x a few microseconds cost less than waking the pool
    const int want = nblocks <= 2 ? 1 : (chain_only || seeds ? nchan : 2 * nchan);
    no_drift = std::getenv("GPSIQ_NO_DRIFT") != nullptr;      // A/B + test knob, read per call: every candidate walked
    verify_every = chain_verify_every();
    const bool trace = std::getenv("GPSIQ_TRACE") != nullptr;
    if (trace && want > 1 && host_threads() < nchan)
        std::fprintf(stderr, "[gpsiq trace] reference NCO: %d host threads for %d channels: pieces are worked through piece-major\n", host_threads(), nchan);
    run_job([](void *p) { static_cast<RefWalk *>(p)->work(); }, this, want);
    for (int i = 0; i < nchan; ++i) { carr_end[i] = carr[i]; last_prn[i] = prev[i]; }
}

int RefWalk::wait_piece(size_t k)
{
    pthread_mutex_lock(&mu);
    while (done[k].load(std::memory_order_acquire) < nchan) pthread_cond_wait(&cv, &mu);
    const int r = rc;
    pthread_mutex_unlock(&mu);
    return r;
}

void RefWalk::take_patches(size_t k, std::vector<gpsiq_patch_t> *out, bool relative)
{
    const uint32_t b0 = k ? (uint32_t) ends[k - 1] : 0u;
    out->clear();
    for (int i = 0; i < nchan; ++i) {
        const std::vector<gpsiq_patch_t> &v = patches[(size_t) i * ends.size() + k];
        out->insert(out->end(), v.begin(), v.end());
    }
    std::sort(out->begin(), out->end(), patch_before);
    if (relative)
        for (gpsiq_patch_t &p : *out) p.block -= b0;
}

void RefWalk::all_patches(std::vector<gpsiq_patch_t> *out)
{
    std::vector<gpsiq_patch_t> part;
    out->clear();
    for (size_t k = 0; k < npieces(); ++k) {
        take_patches(k, &part, false);
        out->insert(out->end(), part.begin(), part.end());
    }
}

}  // namespace gpsiq
