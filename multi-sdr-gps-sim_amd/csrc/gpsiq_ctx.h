// gpsiq_ctx.h -- the device context of libgpsiq (include/gpsiq.h: gpsiq_ctx_t), shared by the translation units of the device half:
// gpsiq_device.cpp (context, resident descriptors, launches, settings), gpsiq_batch.cpp (the drop-in calls of one context),
// gpsiq_multi.cpp (gpsiq_generate_batch_multi) and gpsiq_evaldev.cpp (the batch calls whose descriptors are quantised / evaluated
// on the device), and by the host side of every stream stage.  This header keeps the context itself, the first-use routines of the
// chain and the device evaluation, what the translation units above use of each other, and the synthesis kernels by type.  What a
// stream stage keeps in the context is in that stage's header, included below; what the staged batch calls share (the staging ring
// and the piece loop) is in gpsiq_stage_batch.h, what a stage's single call does around its kernel in gpsiq_stage_call.h; HIP_TRY
// is in gpsiq_own.h.
//
// The files of a stream stage <s> (despread, pack, acquire, follow, filter, spectrum, mix, resample, agc, cfilter, array, stap,
// stap_beams):
//   include/gpsiq_rows.h        the public prototype, and the only place its signature is written outside the definition
//   gpsiq_<s>.h                 the stage's member of gpsiq_ctx (resources, reserve()), its kernels by type and their look-ups,
//                               and `decltype(gpsiq_<s>) gpsiq_<s>_impl;`
//   gpsiq_<s>.cpp               checks, plan, look-up, launch, copy-back: the definition of gpsiq_<s>_impl
//   gpsiq_<s>_plan.h            the plan, pure host arithmetic (pinned on the CPU by the tests)
//   gpsiq_<s>_geometry.h        the constants plan and kernels share              } device sources: in the Makefile's DEVSRC,
//   gpsiq_<s>_kernels.hip       the kernels and the table of those that exist     } behind gpsiq_kernels_id()
//   gpsiq_stream.h              what the kernels of several stages do alike with a stream: sample in, sample out, round and clamp,
//                               count (a device source too); a new stage's kernels take theirs from it
//   gpsiq_stage_call.h          what the calls of several stages do alike around their kernel: the counter and its timed call
//                               (ClipCount, counted_call), check_formats / check_span / check_batch_shape, forced_kernel
//   gpsiq_device.cpp            one line of the gpsiq_plumbing() table: {"<s>", &gpsiq_<s>_impl}
//   gpsiq_rows_link.cpp         the exported gpsiq_<s> of libgpsiq_rows.so: core<decltype(&gpsiq_<s>)>("<s>")
//   gpsiq_stage_math.cpp        its helpers that are plain arithmetic (libgpsiq_rows.so)
//   gpsiq/__init__.py           the Python binding
#ifndef GPSIQ_CTX_H
#define GPSIQ_CTX_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "gpsiq_internal.h"
#include "gpsiq_evalctl.h"
#include "gpsiq_noise.h"
#include "gpsiq_own.h"
#include "gpsiq_pieces.h"
#include "gpsiq_stage_batch.h"
#include "gpsiq_stage_call.h"
#include "gpsiq_despread.h"
#include "gpsiq_pack.h"
#include "gpsiq_acquire.h"
#include "gpsiq_follow.h"
#include "gpsiq_filter.h"
#include "gpsiq_spectrum.h"
#include "gpsiq_mix.h"
#include "gpsiq_resample.h"
#include "gpsiq_agc.h"
#include "gpsiq_cfilter.h"
#include "gpsiq_array.h"
#include "gpsiq_stap.h"
#include "gpsiq_stap_beams.h"

struct gpsiq_ctx {
    template <typename T> using DevBuf = gpsiq::DevBuf<T>;
    template <typename T> using PinnedBuf = gpsiq::PinnedBuf<T>;
    using Event = gpsiq::Event;
    using Stream = gpsiq::Stream;

    int           device = -1;
    Stream        stream;
    Stream        stream2;                               // every other piece of a batch in pieces (piece_stream below)
    DevBuf<gpsiq::DeviceTables> d_tab;
    Stream        copy_stream[2];                        // device-to-host copies of the batch calls
    // resident descriptors, kSets buffers taken in turn: a new set is staged and uploaded into a buffer the latest launches
    // are NOT reading, so gpsiq_set_descriptors never waits for the device to go idle -- only, if it is still in flight, for the
    // launch from kSets sets ago that used the same buffer.  Four: the pieces of a batch alternate between two streams and a
    // piece's kernel shares the device with its neighbour's, so with two sets piece k+2 waited for a piece k that had been
    // slowed down by piece k+1 (GPSIQ_DESC_SETS=2 for the A/B, read per set)
    struct DescBuf {
        DevBuf<gpsiq_qchan_t>    d;                       // device copy, in descriptors
        PinnedBuf<gpsiq_qchan_t> h;                       // page-locked staging of the compacted descriptors
        // one event per stream that has launched on this buffer since it was last known idle: a launch on stream B must
        // not hide a longer one still running on stream A (when more than kUses streams are in play the extra ones
        // are chained behind the first, which then covers them)
        struct Use { hipStream_t s = nullptr; Event ev; bool active = false; };      // (s: the caller's, not ours)
        static constexpr int kUses = 4;
        Use            use[kUses];
        bool           in_use = false;
        std::vector<uint8_t> active_per_block;            // active channels of every resident block (patch validation)
        // patches that go with this set (GPSIQ_NCO_REFERENCE): per buffer, so that the next set's list can be uploaded
        // while launches of this one are still applying theirs
        DevBuf<gpsiq_patch_t>    d_patch;
        int                      npatch = 0;
        PinnedBuf<gpsiq_patch_t> h_patch;                 // page-locked staging of the list (asynchronous sets)
        // a set staged without waiting (the pieces of a batch): the uploads are on up_stream, `uploaded` is recorded behind
        // them, and every launch on the set waits for it on its own stream
        Event          uploaded;
        bool           upload_pending = false;
    } buf[4];
    static constexpr int kSets = 4;
    Stream         up_stream;           // descriptor / patch uploads: never behind a running kernel
    int            cur = 0;             // buf[cur] holds the resident set
    gpsiq_qchan_t *d_desc = nullptr;    // == buf[cur].d.get()
    int            nblocks = 0, nchan = 0;
    gpsiq::SynthClass cls;              // what the resident set contributes to the choice of kernel (gpsiq_launch_plan.h)
    int            nco_mode = GPSIQ_NCO_FIXED;
    // receiver noise (gpsiq_set_noise): on while sigma > 0; next_block is the absolute index the next drop-in call's block 0
    // gets, call_block that of the running call's block 0 (every path of the call numbers its blocks from it).  Settings only:
    // the table they stand for on the context's device is d_noise_tab (gpsiq::noise::kTabEntries)
    struct Noise {
        uint64_t seed = 0, next_block = 0;
        double   sigma = 0.0;
        long     max_z = 0;                            // S_tail[63] = max |z|
    } noise;
    DevBuf<gpsiq::noise::Entry> d_noise_tab;
    uint64_t       call_block = 0;
    // output level stage (gpsiq_set_level, include/gpsiq_rows.h): on while mult != 0.  d_zero_tab is the all-zero noise table the
    // kernels read while the level is on and the noise is off
    struct Level {
        uint32_t mult = 0;
        int32_t  qmax = 0;
    } level;
    DevBuf<gpsiq::noise::Entry> d_zero_tab;
    // scratch of the kernel variants that need some (segm: the sign masks of one launch), in bytes
    DevBuf<uint8_t> d_scratch;
    // staging of the batch calls' output (PieceOut below), in bytes
    DevBuf<uint8_t> d_out;
    Event           chunk_done[2];
    // gpsiq_generate_block_async: a small ring of per-block descriptor / output staging, each with the event that
    // says its block has landed.  Every member is reserved / ensured on its own by every call: a call that failed half-way
    // leaves nothing that looks complete
    struct AsyncSlot {
        DevBuf<gpsiq_qchan_t>    d;
        PinnedBuf<gpsiq_qchan_t> h;
        DevBuf<gpsiq_patch_t>    d_patch;                 // GPSIQ_NCO_REFERENCE: the block's patches ...
        PinnedBuf<gpsiq_patch_t> h_patch;                 // ... staged page-locked
        DevBuf<uint8_t>          out;                     // bytes
        Event          done;
        bool           busy = false;
    } aslot[4];
    int anext = 0;
    // carrier carry per slot (gpsiq_generate_block): one value, so that a call can put it back and a change of model forgets it
    struct Carry { uint64_t phase[GPSIQ_MAX_CHAN] = {}; double handed[GPSIQ_MAX_CHAN] = {}; int prn[GPSIQ_MAX_CHAN] = {}; } carry;
    // GPSIQ_NCO_REFERENCE batch calls: quantised descriptors and start states of the timeline being worked through, kept
    // between calls (a fresh 1.5 MB per call is four hundred page faults on the thread everything else waits for)
    std::vector<gpsiq_qchan_t> ref_q;
    std::vector<double>        ref_start;
    // gpsiq_generate_batch with descriptors in the context's device memory and the host path about to read them: the rows, copied
    // down once per call, page-locked (gpsiq_batch.cpp: rows_to_host)
    PinnedBuf<gpsiq_chan_t>    h_rows;
    // the carrier chain of GPSIQ_NCO_REFERENCE on the device (gpsiq_chain_maps_device): inputs, estimates and maps of the
    // timeline being worked through, device side and page-locked staging, kept between calls
    struct Chain {
        DevBuf<gpsiq_chain_in_t>     d_in;              // these five hold the same number of blocks x channels (reserve)
        PinnedBuf<gpsiq_chain_in_t>  h_in;
        DevBuf<uint8_t>              d_prep;            // lane::Prep, kPrepBytes each
        DevBuf<gpsiq_chain_map_t>    d_maps;
        PinnedBuf<gpsiq_chain_map_t> h_maps;
        DevBuf<gpsiq_chain_est_t>    d_est;             // [kEvalMaxPieces + 1][GPSIQ_MAX_CHAN]: start, end of the first launch (= start of a second), end
        PinnedBuf<gpsiq_chain_est_t> h_est;
        DevBuf<double>               d_c_before;
        Stream             stream, back;                // uploads + kernels; the maps' way back + the callbacks (never in the kernels' way)
        Event              t0, t1, landed;              // landed: the maps of the last range queued are in h_maps
        Event              walked[2];                   // a launch's kernels are done
        float              last_ms = 0.0f;              // device time of the last call's two kernels
        static constexpr size_t kPrepBytes = 32;
        int reserve(size_t n);                          // first use + room for n blocks x channels
    } chain;
    // batch calls whose descriptors are quantised / evaluated on the device (gpsiq_evaldev.cpp; shares chain's buffers and streams)
    struct EvalDev {
        static constexpr size_t kChanBytes = 64;        // sizeof(ev::DChan) (gpsiq_eval.h)
        static constexpr unsigned kPatchCap = 1u << 16, kHostCap = 1u << 13;
        DevBuf<uint8_t>    d_chan;                      // ev::DChan rows, in bytes: device ...
        PinnedBuf<uint8_t> h_chan;                      // ... and page-locked staging (host-packed sources), the same size
        DevBuf<gpsiq_chan_t> d_raw;                     // page-locked sources: the raw descriptors in HBM
        DevBuf<double>     d_seeds;                     // start states given by the caller (gpsiq_generate_seeded)
        DevBuf<gpsiq::EvalCtrl>    d_ctrl;
        PinnedBuf<gpsiq::EvalCtrl> h_ctrl;              // [kEvalMaxPieces + 2]: a snapshot behind every piece, one at the end, the zeroed one
        DevBuf<gpsiq::LinkCarry>   d_link;  PinnedBuf<gpsiq::LinkCarry>  h_link;     // [GPSIQ_MAX_CHAN]
        DevBuf<gpsiq::FixedCarry>  d_fix;   PinnedBuf<gpsiq::FixedCarry> h_fix;
        DevBuf<gpsiq_patch_t>      d_patches;  PinnedBuf<gpsiq_patch_t>  h_patches;  // [kPatchCap]
        DevBuf<gpsiq::EvalHostItem> d_host;  PinnedBuf<gpsiq::EvalHostItem> h_host;  // [kHostCap]
        PinnedBuf<gpsiq_chan_t>    h_items;             // device-resident descriptors the host walker needs, page-locked
        DevBuf<gpsiq::EvalSlotRow> d_slot;  PinnedBuf<gpsiq::EvalSlotRow> h_slot;    // repair: one slot's column (+ one row before), device and page-locked
        DevBuf<double>     d_col;  PinnedBuf<double> h_col;                          // ... and its start states on the way back (one size, reserve_repair)
        Stream             eval_stream, chain_stream;   // highest priority: beside the synthesis, ahead of its workgroups
        Event              linked[gpsiq::kEvalMaxPieces], evaluated[gpsiq::kEvalMaxPieces], joined, t_synth0, t_synth1;
        // statistics of the last call (gpsiq_evaldev_stats)
        double          host_ms = 0.0;                 // host thread-time spent on the call's descriptors (pack, repair, walker)
        unsigned        last_nhost = 0, last_npatch = 0, last_repaired = 0;
        int reserve(size_t n, bool pinned_source, bool seeds);     // first use + room for n blocks x channels
        int reserve_repair(size_t rows);
    } evd;
    // the stream stages, each in the header of its name: gpsiq_despread; gpsiq_pack / gpsiq_unpack / gpsiq_generate_batch_packed;
    // gpsiq_acquire; gpsiq_follow; gpsiq_filter / gpsiq_generate_batch_filtered; gpsiq_spectrum;
    // gpsiq_mix / gpsiq_generate_batch_mixed; gpsiq_resample / gpsiq_generate_batch_resampled; gpsiq_agc / gpsiq_generate_batch_agc;
    // gpsiq_cfilter; gpsiq_array_cov / gpsiq_array_combine; gpsiq_stap_cov / gpsiq_stap_combine;
    // gpsiq_stap_beams
    gpsiq::DespreadSet dsp;
    gpsiq::PackSet     pack;
    gpsiq::AcquireSet  acq;
    gpsiq::FollowSet   fol;
    gpsiq::FirSet      filt;
    gpsiq::SpectrumSet spec;
    gpsiq::MixSet      mix;
    gpsiq::ResampleSet rs;
    gpsiq::AgcSet      agc;
    gpsiq::FirSet      cfilt;               // (its own: nothing is shared between the two filters at run time)
    gpsiq::ArraySet    array;
    gpsiq::StapSet     stap;
    gpsiq::BeamsSet    beams;
    // the staging the five staged batch calls (_packed, _filtered, _mixed, _resampled, _agc) work through their pieces with: one ring for
    // all of them -- calls on a context are serial and every one ends with the ring's streams drained (gpsiq_stage_batch.h)
    gpsiq::PieceRing   ring;
};

// ---- first use and growth of the chain's and the device evaluation's resources (the rule: reserve_together, gpsiq_own.h) ------
inline int gpsiq_ctx::Chain::reserve(size_t n)
{
    // (equal priorities: with the synthesis stream above the chain's, the second launch's maps came back late -- 0.98 ms
    // instead of 0.78 -- and the pieces behind the head waited for them: 2.6 ms per call instead of 2.4, profiles/r05_chain_ab.txt)
    HIP_TRY(stream.ensure());
    HIP_TRY(back.ensure());
    for (auto &e : walked) HIP_TRY(e.ensure());
    HIP_TRY(t0.ensure(hipEventDefault));
    HIP_TRY(t1.ensure(hipEventDefault));
    HIP_TRY(landed.ensure());
    HIP_TRY(d_est.reserve((gpsiq::kEvalMaxPieces + 1) * GPSIQ_MAX_CHAN));
    HIP_TRY(h_est.reserve((gpsiq::kEvalMaxPieces + 1) * GPSIQ_MAX_CHAN));
    HIP_TRY(d_c_before.reserve(gpsiq::kEvalMaxPieces * GPSIQ_MAX_CHAN));
    // (reserve_together's rule in lines of its own: d_prep counts in bytes, kPrepBytes per entry, its neighbours in entries, and it
    // keeps its place in the order the five are grown in)
    if (n <= std::min({d_in.cap(), h_in.cap(), d_prep.cap() / kPrepBytes, d_maps.cap(), h_maps.cap()})) return GPSIQ_OK;
    const size_t cap = n + n / 4 + 256;
    HIP_TRY(d_in.reserve(cap));
    HIP_TRY(h_in.reserve(cap));
    HIP_TRY(d_prep.reserve(cap * kPrepBytes));
    HIP_TRY(d_maps.reserve(cap));
    HIP_TRY(h_maps.reserve(cap));
    return GPSIQ_OK;
}

inline int gpsiq_ctx::EvalDev::reserve(size_t n, bool pinned_source, bool seeds)
{
    // Chain and evaluation run BESIDE the synthesis, which floods the device with workgroups: their streams get the highest
    // priority, so that the few workgroups of prepare / lanes / link / evaluation are dispatched as synthesis workgroups retire
    // instead of behind all of them (the patches have to be there when the synthesis ends, not some time after it).
    // (MI355X, 2.6 Msps, 2 000 blocks: 1.82 ms per call against 2.20 at equal priorities; 25 Msps: 1.54 against 2.61)
    HIP_TRY(eval_stream.ensure_greatest());
    HIP_TRY(chain_stream.ensure_greatest());
    HIP_TRY(t_synth0.ensure(hipEventDefault));
    HIP_TRY(t_synth1.ensure(hipEventDefault));
    for (auto &ev_ : linked) HIP_TRY(ev_.ensure());
    for (auto &ev_ : evaluated) HIP_TRY(ev_.ensure());
    HIP_TRY(joined.ensure());
    HIP_TRY(d_ctrl.reserve(1));
    HIP_TRY(h_ctrl.reserve(gpsiq::kEvalMaxPieces + 2));
    HIP_TRY(d_link.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(h_link.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(d_fix.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(h_fix.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(d_patches.reserve(kPatchCap));
    HIP_TRY(h_patches.reserve(kPatchCap));
    HIP_TRY(d_host.reserve(kHostCap));
    HIP_TRY(h_host.reserve(kHostCap));
    HIP_TRY(gpsiq::reserve_together(n * kChanBytes, (n + n / 4 + 256) * kChanBytes, d_chan, h_chan));       // both in bytes
    if (pinned_source) HIP_TRY(gpsiq::reserve_together(n, n + n / 4 + 16, d_raw));
    if (seeds) HIP_TRY(gpsiq::reserve_together(n, n + n / 4 + 16, d_seeds));
    return GPSIQ_OK;
}

inline int gpsiq_ctx::EvalDev::reserve_repair(size_t rows)
{
    HIP_TRY(gpsiq::reserve_together(rows, rows + 256, d_slot, h_slot, d_col, h_col));
    return GPSIQ_OK;
}

// ---- what the translation units of the device half use of each other ----------------------------------------------------------
// gpsiq_device.cpp:
// the noise and the output level of launches whose descriptor array starts at absolute block `block` (tab == nullptr while both are off)
gpsiq::noise::Launch gpsiq_noise_at(const gpsiq_ctx *c, uint64_t block);
double gpsiq_wall_ms();                                         // GPSIQ_TRACE: host-side phase times
int gpsiq_wait_idle(gpsiq_ctx::DescBuf &b);                     // until no launch reads the set any more
int gpsiq_mark_use(gpsiq_ctx::DescBuf &b, hipStream_t s);       // stream s has just launched work reading the set
// gpsiq_set_descriptors with the set's patches in the same step; no_wait: the uploads are queued, launches wait for them on the device
int gpsiq_stage_descriptors(gpsiq_ctx_t *c, const gpsiq_qchan_t *q, int nblocks, int nchan, const gpsiq_patch_t *patches, int npatch, bool no_wait);
// gpsiq_launch with the absolute block index of the resident set's block 0 (receiver noise) given by the caller
int gpsiq_launch_abs(gpsiq_ctx *c, int block0, int nblocks, int nsamp, int sample_size, void *dst, size_t stride, hipStream_t s, int variant, uint64_t nbase);
// seed and sigma / the level of a context, checked by the caller (gpsiq_generate_batch_multi lends context 0's); the counter stays
int gpsiq_apply_noise(gpsiq_ctx *c, uint64_t seed, double sigma);
int gpsiq_apply_level(gpsiq_ctx *c, uint32_t mult, int32_t qmax);
// the clamp has to fit the format, which only a rendering call knows
inline int gpsiq_check_level(const gpsiq_ctx *c, int sample_size)
{
    if (c->level.mult && c->level.qmax > (sample_size == GPSIQ_SC08 ? 127 : 32767))
        return gpsiq::fail(GPSIQ_E_ARG, "output level: qmax %d does not fit %d-byte samples", (int) c->level.qmax, sample_size);
    return GPSIQ_OK;
}
// The stream of piece k of a batch worked through in pieces.  On ONE stream a piece's kernel starts when the last workgroup of
// the piece before it has retired: every piece pays its own ramp-down (six pieces of a 2 000-block call: 1.75 ms of kernels
// against 1.50 ms in one launch, profiles/r05_chain_ab.txt).  Pieces write disjoint blocks and read their own descriptor set
// (four sets taken in turn; piece k+2 follows piece k on the same stream), so consecutive pieces alternate
// between two streams and the next piece's first workgroups fill the compute units the last ones of this piece leave.
// (One stream against two: profiles/r05_chain_ab.txt.)
inline hipStream_t gpsiq_piece_stream(gpsiq_ctx *c, int k) { return ((k & 1) ? c->stream2 : c->stream).get(); }

// The output of one batch call: its blocks are rendered straight into the caller's device memory where the rows are ours
// (direct: 16-byte rows, 4-byte aligned), else into c->d_out with 16-byte rows and copied across on the context's two copy
// streams, in turn.  finish() is the call's one drain: on every path, also after an error, nothing may still write dst or
// read the staging when the call returns.
struct PieceOut {
    gpsiq_ctx *c = nullptr;
    uint8_t   *dst = nullptr;
    size_t     blk_bytes = 0, stride = 0;      // bytes of a block, and between blocks as rendered
    int        nblocks = 0, copies = 0;
    bool       dst_is_device = false, direct = false;

    int begin(gpsiq_ctx *ctx, int nblocks, int nsamp, int sample_size, void *dst, int dst_is_device);   // sizes the staging
    uint8_t *target(int b0) const { return (direct ? dst : c->d_out.get()) + (size_t) b0 * stride; }   // where block b0 is rendered
    int rendered(int b0, int nb, hipStream_t s);                 // blocks [b0, b0 + nb) cross once their kernel on s is done
    int whole(hipStream_t s);                                    // every block, behind the kernel on s (one kernel, one copy)
    int again(hipStream_t s, const std::vector<gpsiq_patch_t> &patches);   // the blocks patched on s (sorted by block) once more
    int finish(const char *label, int rc = GPSIQ_OK);            // rc != GPSIQ_OK: the call has failed, its error text stands
};

// gpsiq_batch.cpp: piece k of a GPSIQ_NCO_REFERENCE range, blocks [b0, b0 + nb) of it, queued without waiting
int gpsiq_ref_piece(gpsiq_ctx *c, PieceOut &out, int k, const gpsiq_qchan_t *q, int b0, int nb, int nchan, int nsamp, int ss, uint64_t nbase,
                    const std::vector<gpsiq_patch_t> &patches);

// what a patch list of n entries (n > 0) asks its buffers for
inline size_t gpsiq_patch_room(size_t n) { return n < 256 ? 256 : n; }

// the fixed-point carrier: whether slot i continues what the context handed out (the caller gave back what it was given) ...
inline bool gpsiq_continues(const gpsiq_ctx *c, int i, const gpsiq_chan_t &ch)
{
    return ch.prn > 0 && c->carry.prn[i] == ch.prn && c->carry.handed[i] == ch.carr_phase;
}
// ... and what a batch call leaves in slot i: satellite prn (0: none) with the accumulator at `phase`
inline void gpsiq_hand_back(gpsiq_ctx *c, int i, int prn, uint64_t phase, double *carr_phase_out)
{
    c->carry.prn[i] = prn;
    c->carry.phase[i] = prn ? phase : 0;
    c->carry.handed[i] = prn ? gpsiq::carr_phase_to_double(phase) : 0.0;
    if (carr_phase_out) carr_phase_out[i] = c->carry.handed[i];
}

// gpsiq_batch.cpp:
int gpsiq_check_gen_args(const gpsiq_ctx *c, const void *ch, const void *dst, int nblocks, int nchan, int nsamp, double fs, int sample_size);
// quantised blocks q[0, nblocks) to dst: set resident, rendered, copied (nbase: absolute block index of q[0], for the receiver noise)
int gpsiq_run_to_host_or_device(gpsiq_ctx *c, const gpsiq_qchan_t *q, int nblocks, int nchan, int nsamp, int sample_size, void *dst, int dst_is_device, uint64_t nbase);
double gpsiq_rate_kernel();                                     // channel-samples per second of the synthesis kernel: measured, else MI355X's
void gpsiq_note_kernel_rate(double channel_samples_per_s);      // a measured rate of the synthesis kernel (running mean)
// GPSIQ_NCO_REFERENCE batch with chain link and evaluation on host threads (the path of rounds 4-5; fallback of the device path)
int gpsiq_generate_reference_host(gpsiq_ctx *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs,
                                  int sample_size, void *dst, int dst_is_device, double *carr_phase_out, const double *seeds = nullptr);
// level 1 of the carrier chain on the device: whether a batch takes it, the inputs of blocks [b0, b1) staged, the staged blocks' maps waited for
bool gpsiq_chain_on_device(int nblocks, int nsamp, int nchan);
void gpsiq_chain_stage_inputs(gpsiq_ctx *c, const gpsiq_chan_t *ch, int b0, int b1, int nchan);
int gpsiq_chain_maps_staged(gpsiq_ctx *c, int nblocks, int nchan, double fs, int nsamp, const gpsiq_chain_est_t *start, int max_stretches,
                            gpsiq_chain_est_t *end);
// Where a call's descriptors lie.  gpsiq_rows_kind is the one place that asks the runtime, once per call, at the call's entry and
// before anything is queued: host memory the runtime does not know is pageable (it is not probed), device memory of the context's
// device is kSrcDevice, and what neither the host nor that device can read (another device's memory, a HIP array) is GPSIQ_E_ARG
// with the kind of pointer in the text.  host_call: the name of a call that reads ch on the host by contract
// (gpsiq_generate_seeded, gpsiq_generate_batch_multi, gpsiq_generate_batch_packed) -- device memory is GPSIQ_E_ARG there too.
namespace gpsiq { enum SrcKind { kSrcPageable = 0, kSrcPinned = 1, kSrcDevice = 2 }; }
int gpsiq_rows_kind(const gpsiq_ctx *c, const void *ch, const char *host_call, gpsiq::SrcKind *kind);
// gpsiq_evaldev.cpp: the same call (either NCO model) with the descriptors quantised / evaluated on the device.  *handled = 0:
// not taken (too short a batch, switched off, or its lists overflowed), the caller goes on with the host path -- which reads ch
// on the host: rows of kSrcDevice are the caller's to copy down first
int gpsiq_generate_device(gpsiq_ctx *c, const gpsiq_chan_t *ch, gpsiq::SrcKind kind, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                          void *dst, int dst_is_device, double *carr_phase_out, const double *seeds, int *handled);

namespace gpsiq {
// The synthesis kernels by type (gpsiq_kernels.hip holds them and the table of the instantiations that exist; a lookup returns
// nullptr where there is none).  Common head: descriptors, nchan, nsamp, dst, block stride, block0, tables.
using TileFn      = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, int, int, int, int, int);
using TileNoiseFn = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, int, int, int, int, int,
                             const noise::Entry *, uint64_t, uint64_t);
using TileLevelFn = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, int, int, int, int, int,
                             const noise::Entry *, uint64_t, uint64_t, uint32_t, int32_t);
using MaskFn      = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, const uint64_t *, int, int, int);
using SignMasksFn = void (*)(const gpsiq_qchan_t *, int, int, int, int, const DeviceTables *, uint64_t *, int, int);
using RowsFn      = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, int);
using GenericFn   = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, const DeviceTables *, int, int,
                             const noise::Entry *, uint64_t, uint64_t, uint32_t, int32_t);
using PatchFn     = void (*)(const gpsiq_qchan_t *, int, int, uint8_t *, size_t, int, int, const DeviceTables *, const gpsiq_patch_t *, int,
                             const noise::Entry *, uint64_t, uint64_t, uint32_t, int32_t);
TileFn      tile_kernel(int fmt, int slots, bool half, bool fast);          // tile, seg (half = false), segh
TileNoiseFn tile_noise_kernel(int fmt, int slots, bool half, bool fast);
TileLevelFn tile_level_kernel(int fmt, int slots, bool half, bool fast);
TileFn      both_kernel(int fmt, int slots);                                // segb
MaskFn      mask_kernel(int fmt, int slots);                                // segm, behind sign_masks_kernel()
SignMasksFn sign_masks_kernel();
RowsFn      rowsx_kernel(int fmt, int slots);
RowsFn      rows_kernel(int fmt);
GenericFn   generic_kernel(int fmt);
PatchFn     patch_kernel(int fmt);

// gpsiq_launch.cpp: the one door every rendered sample goes through.  cls: what the descriptors at desc contribute to the choice
// of kernel (gpsiq_launch_plan.h); variant: not kAuto (auto_variant() resolves it)
hipError_t launch_variant(int variant, const gpsiq_qchan_t *desc, int nchan, int nsamp, int sample_size,
                          void *dst, size_t block_stride, int block0, int nblocks,
                          const DeviceTables *tab, hipStream_t stream, const SynthClass &cls, void *scratch,
                          const noise::Launch &nz);
hipError_t launch_patches(const gpsiq_qchan_t *desc, int nchan, int nsamp, int sample_size, void *dst, size_t block_stride,
                          int block0, int nblocks, const DeviceTables *tab, const gpsiq_patch_t *patches, int npatch,
                          hipStream_t stream, const noise::Launch &nz);
hipError_t launch_chain(const void *d_in, int in_stride, int nblocks, int nchan, double delt, int nsamp, const gpsiq_chain_est_t *d_start,
                        int max_seg, void *d_prep, double *d_c_before, gpsiq_chain_est_t *d_end, void *d_maps, hipStream_t stream, int which = 3);
int chain_link(const gpsiq_chain_in_t *in, const void *maps, int nblocks, int nchan, double delt, int nsamp,
               const double *carr_in, const int32_t *prn_in, double *carr_start, double *carr_end, int32_t *last_prn);
double chain_block_true(double f_carr, double delt, int nsamp, double start);
}
#endif
