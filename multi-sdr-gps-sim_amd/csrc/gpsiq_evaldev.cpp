// gpsiq_evaldev.cpp -- gpsiq_generate_batch / gpsiq_generate_seeded with the descriptors quantised and, in GPSIQ_NCO_REFERENCE,
// chained and evaluated ON THE DEVICE (kernels: gpsiq_chain_kernels.hip, gpsiq_eval_kernels.hip; the lane code: gpsiq_eval.h).
//
// What the reference's host code leaves per block and channel at gps.c:2766 (gpsiq_chan_t) goes in; per piece of the batch
//     pack -> [chain_prepare -> chain_lanes -> chain_link_scan] -> eval_blocks | quantize_fixed -> synth_tile (-> apply_patches)
// with no host stage between them.  What the host still does:
//   * descriptors in PAGEABLE host memory are cut down to 64 bytes each on the pool (the device cannot read them; page-locked
//     and device-resident descriptors are read where they lie);
//   * it waits for each piece's link (an event, the device busy with the pieces behind) to learn the synthesis kernel's launch
//     parameters and whether a slot has a block whose certified map does not apply -- then that slot's chain is walked by the host
//     walker (lane::link_block + the true walk, as rounds 4-5 did for every slot) and its start states go back up;
//   * the (block, channel) pairs whose candidates the drift enclosure cannot decide (1 in 10^4) get the host evaluation
//     (eval_block) while the device renders, and the merged, sorted patch list goes up before apply_patches.
// Results are those of the host path (gpsiq_generate_reference_host / the host quantiser) bit for bit: tests/eval_twin.cpp on
// the CPU, tests/test_gpu_device_eval.py and every T2 = 0 test on the GPU.
// Reference lines: gps.c:2033-2064 (what the quantiser takes in), 2775-2782 (index + truncation), 2789-2826 (the accumulators),
// 2208-2214 (re-seeding a slot).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_eval.h"
#include "gpsiq_pieces.h"

using namespace gpsiq;

namespace gpsiq {
// gpsiq_exact.cpp: one channel of one block on the host (descriptor + patches from its start state)
int eval_block_host(const gpsiq_chan_t &ch, double start, const uint64_t *seed, double delt, int nsamp, int block, int slot, gpsiq_qchan_t *q,
                    std::vector<gpsiq_patch_t> *out);
}

namespace {

static_assert(sizeof(ev::DChan) == gpsiq_ctx::EvalDev::kChanBytes, "the rows d_chan / h_chan are sized for");
constexpr unsigned kPatchCap = gpsiq_ctx::EvalDev::kPatchCap, kHostCap = gpsiq_ctx::EvalDev::kHostCap;

// descriptors in pageable memory: cut down to ev::DChan on the pool, with the synthesis kernel's launch parameters on the way
struct PackJob { const gpsiq_chan_t *ch; ev::DChan *out; const double *seeds; int nchan; double delt; uint64_t mx; int max_active; long max_amp; };
void pack_host(PackJob *pj, int nblocks)
{
    parallel_for(nblocks, 0, 64, [](void *p, int b0, int b1) {
        PackJob &j = *static_cast<PackJob *>(p);
        uint64_t mx = 0;
        int max_active = 0;
        long max_amp = 0;
        for (int b = b0; b < b1; ++b) {
            int na = 0;
            long amp = 0;
            for (int i = 0; i < j.nchan; ++i) {
                const size_t k = (size_t) b * j.nchan + i;
                if (b + 1 < b1) __builtin_prefetch(reinterpret_cast<const char *>(&j.ch[k + j.nchan]));
                ev::DChan d;
                ev::pack_chan(j.ch[k], &d);
                if (j.seeds) d.start = j.seeds[k];
                j.out[k] = d;
                const double code_inc = d.f_code * j.delt;
                if (d.prn > 0 && d.prn <= 32 && code_inc > 0.0 && code_inc < 2.0 && d.gain > -ev::kEvMaxGain && d.gain < ev::kEvMaxGain) {
                    const uint64_t cs = (uint64_t) (int64_t) __builtin_rint(code_inc * 0x1p56);
                    if (cs > mx) mx = cs;
                    amp += (long) (250.0 * std::fabs(d.gain));
                    ++na;
                }
            }
            if (na > max_active) max_active = na;
            if (amp > max_amp) max_amp = amp;
        }
        for (uint64_t cur = j.mx; mx > cur && !__sync_bool_compare_and_swap(&j.mx, cur, mx); cur = j.mx) {}
        for (int cur = j.max_active; max_active > cur && !__sync_bool_compare_and_swap(&j.max_active, cur, max_active); cur = j.max_active) {}
        for (long cur = j.max_amp; max_amp > cur && !__sync_bool_compare_and_swap(&j.max_amp, cur, max_amp); cur = j.max_amp) {}
    }, pj);
}

// one slot's chain on the host through the device's maps (link_slot of gpsiq_chain.cpp on the slot's gathered column), blocks
// [b0, b1): rows[b - b0]; every start state -> start_col[b - b0]; *x / *pv: the accumulator and satellite before block b0
// (b0 > 0), and after block b1 - 1 on return.  false: a state or Doppler outside the NCO format (*bad_block)
bool link_slot_host(const EvalSlotRow *rows, int b0, int b1, double delt, int nsamp, double *x_io, int *pv_io, double *start_col,
                    long *linked, long *walked, int *bad_block)
{
    static_assert(sizeof(gpsiq_chain_map_t) == sizeof(lane::Rec), "the map as the lanes write it");
    double x = *x_io;
    int pv = *pv_io;
    for (int b = b0; b < b1; ++b) {
        const EvalSlotRow &d = rows[b - b0];
        if (d.prn <= 0) { pv = 0; x = 0.0; start_col[b - b0] = 0.0; continue; }
        if (b == 0 || pv != d.prn) x = d.carr_phase;
        pv = d.prn;
        start_col[b - b0] = x;
        const double inc = d.f_carr * delt;
        if (!(x >= 0.0 && x <= 1.0) || !(std::fabs(inc) < 0.5)) { *bad_block = b; return false; }
        double y;
        if (lane::link_block(*reinterpret_cast<const lane::Rec *>(&d.map), x, &y)) { x = y; ++*linked; }
        else { x = chain_block_true(d.f_carr, delt, nsamp, x); ++*walked; }
    }
    *x_io = x; *pv_io = pv;
    return true;
}

bool patch_before(const gpsiq_patch_t &a, const gpsiq_patch_t &b)
{
    if (a.block != b.block) return a.block < b.block;
    if (a.sample != b.sample) return a.sample < b.sample;
    return a.slot < b.slot;
}

}  // namespace

namespace gpsiq { void chain_count(long linked, long walked); }

static uint64_t g_evd_stats[6];       // calls, (block, channel) pairs evaluated on the device, handed to the host walker, slots repaired, patches, calls that fell back

extern "C" void gpsiq_device_eval_stats(uint64_t out[6])
{
    if (!out) return;
    for (int k = 0; k < 6; ++k) out[k] = __atomic_load_n(&g_evd_stats[k], __ATOMIC_RELAXED);
}

extern "C" double gpsiq_device_eval_host_ms(const gpsiq_ctx_t *c) { return c ? c->evd.host_ms : 0.0; }

// how many entries the patch / host lists of a call may hold.  (-DGPSIQ_TEST_HOOKS: GPSIQ_TEST_LIST_CAP=n makes the lists n entries
// short, so that a test can see what a call does when they overflow -- the whole call again on the host path.)
static inline unsigned list_cap(unsigned cap)
{
#ifdef GPSIQ_TEST_HOOKS
    if (const char *s = std::getenv("GPSIQ_TEST_LIST_CAP")) { const long v = std::atol(s); if (v >= 0 && (unsigned long) v < cap) return (unsigned) v; }
#endif
    return cap;
}

// Whether the device path takes a batch: long enough for its fixed costs (a dozen launches, two or three waits: ~0.06 ms) to pay.
// GPSIQ_NCO_REFERENCE: from 48 blocks (measured, 2.6 and 25 Msps, 16 host threads: the host path is ahead below that).  Fixed-point
// model: the host quantiser costs ~0.2 us per descriptor and thread, so the device takes over at ~300 descriptors per host thread
// (16 threads: 300 blocks of 16 channels; two threads: 38).  GPSIQ_EVAL=host / device decides by hand (read per call).
static bool device_path_wanted(const gpsiq_ctx *c, int nblocks, int nchan)
{
    const char *e = std::getenv("GPSIQ_EVAL");
    if (e && !std::strcmp(e, "host")) return false;
    if (e && !std::strcmp(e, "device")) return nblocks >= 1;
    if (std::getenv("GPSIQ_CHAIN")) return false;          // where level 1 of the chain runs WITHIN the host evaluation: asks for that path
    if (c->nco_mode == GPSIQ_NCO_REFERENCE) return nblocks >= 48;
    return (long) nblocks * nchan >= 300L * (host_threads() > 0 ? host_threads() : 1);
}

// (kind: where ch lies, as the call's entry classified it -- gpsiq_rows_kind, gpsiq_batch.cpp)
int gpsiq_generate_device(gpsiq_ctx *c, const gpsiq_chan_t *ch, SrcKind kind, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                          void *dst, int dst_is_device, double *carr_phase_out, const double *seeds, int *handled)
{
    *handled = 0;
    if (!device_path_wanted(c, nblocks, nchan) || nsamp <= 0) return GPSIQ_OK;
    const bool reference = c->nco_mode == GPSIQ_NCO_REFERENCE || seeds != nullptr;
    const char *trace_env = std::getenv("GPSIQ_TRACE");
    const bool trace = trace_env != nullptr;
    const double t0 = gpsiq_wall_ms();
    HIP_TRY(hipSetDevice(c->device));
    gpsiq_ctx::EvalDev &e = c->evd;
    const size_t n = (size_t) nblocks * (size_t) nchan;
    const double delt = 1.0 / fs;
    const void *dev_src = kind == kSrcDevice ? ch : nullptr;
    int rc = c->chain.reserve(n);
    if (rc == GPSIQ_OK) rc = e.reserve(n, kind == kSrcPinned, seeds != nullptr);
    if (rc) return rc;
    *handled = 1;
    __atomic_fetch_add(&g_evd_stats[0], 1, __ATOMIC_RELAXED);
    e.host_ms = 0.0; e.last_nhost = 0; e.last_npatch = 0; e.last_repaired = 0;
    double host_part[3] = {0.0, 0.0, 0.0};               // pack of pageable rows, repair of slots, patch lists + the host walker's share (the trace's business)

    // the first and the last block's descriptors on the host: the continuation test of the fixed model, the phase handed out for
    // a slot that ends unused
    std::vector<gpsiq_chan_t> edge;
    const gpsiq_chan_t *first = ch, *last = ch + (size_t) (nblocks - 1) * nchan;
    if (kind == kSrcDevice) {
        edge.resize((size_t) 2 * nchan);
        HIP_TRY(hipMemcpy(edge.data(), ch, (size_t) nchan * sizeof(gpsiq_chan_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(edge.data() + nchan, last, (size_t) nchan * sizeof(gpsiq_chan_t), hipMemcpyDeviceToHost));
        first = edge.data(); last = edge.data() + nchan;
    }

    // destination: straight into the caller's device memory where its rows are ours, else through the context's staging
    PieceOut out;
    rc = out.begin(c, nblocks, nsamp, sample_size, dst, dst_is_device);
    if (rc) return rc;

    // the descriptor set the evaluation writes and the synthesis reads: one for the whole call
    int nsets = gpsiq_ctx::kSets;
    const int next = (c->cur + 1) % nsets;
    gpsiq_ctx::DescBuf &nb_ = c->buf[next];
    rc = gpsiq_wait_idle(nb_);
    if (rc) return rc;
    HIP_TRY(nb_.d.reserve(n));

    std::vector<int> ends;
    device_piece_ends(nblocks, nsamp, nchan, kind != kSrcDevice, reference, gpsiq_rate_kernel(), piece_blocks_env(), kEvalMaxPieces, &ends);
    const int npieces = (int) ends.size();
    hipStream_t S = e.chain_stream.get(), E = e.eval_stream.get();
    ev::DChan *d_chan = reinterpret_cast<ev::DChan *>(e.d_chan.get()), *h_chan = reinterpret_cast<ev::DChan *>(e.h_chan.get());
    // the rest of what the call works in, under the names of its owners (reserved above, nothing grows before the repair)
    gpsiq_qchan_t *const d_set = nb_.d.get();
    const DeviceTables *const d_tab = c->d_tab.get();
    gpsiq::EvalCtrl *const d_ctrl = e.d_ctrl.get(), *const h_ctrl = e.h_ctrl.get();
    gpsiq::LinkCarry *const d_link = e.d_link.get(), *const h_link = e.h_link.get();
    gpsiq::FixedCarry *const d_fix = e.d_fix.get(), *const h_fix = e.h_fix.get();
    gpsiq_patch_t *const d_patches = e.d_patches.get(), *const h_patches = e.h_patches.get();
    gpsiq::EvalHostItem *const d_host = e.d_host.get(), *const h_host = e.h_host.get();
    gpsiq_chan_t *const d_raw = e.d_raw.get();
    double *const d_seeds = e.d_seeds.get(), *const d_c_before = c->chain.d_c_before.get();
    uint8_t *const d_prep = c->chain.d_prep.get();
    gpsiq_chain_est_t *const d_est = c->chain.d_est.get();
    gpsiq_chain_map_t *const d_maps = c->chain.d_maps.get();

    // ---- phase A: per piece stage the rows, estimate (chain_prepare), quantise from the estimate, render ------------------------
    // The synthesis of a piece waits for nothing but its own descriptors: in GPSIQ_NCO_REFERENCE they are seeded from
    // chain_prepare's ESTIMATE of every block's start state (good to ~1e-11 cycle), and what the double path from the TRUE start
    // state does differently goes into the patch list when the chain has been linked (phase B), beside the running synthesis.
    EvalCtrl zero;
    std::memset(&zero, 0, sizeof zero);
    zero.err_key = ~0ull;
    h_ctrl[kEvalMaxPieces + 1] = zero;
    HIP_TRY(hipMemcpyAsync(d_ctrl, &h_ctrl[kEvalMaxPieces + 1], sizeof(EvalCtrl), hipMemcpyHostToDevice, S));
    bool cont0[GPSIQ_MAX_CHAN] = {};
    if (!reference) {
        for (int i = 0; i < nchan; ++i) {
            cont0[i] = gpsiq_continues(c, i, first[i]);
            h_fix[i].phase = c->carry.phase[i]; h_fix[i].prn = c->carry.prn[i]; h_fix[i].cont = cont0[i] ? 1 : 0;
        }
        HIP_TRY(hipMemcpyAsync(d_fix, h_fix, (size_t) nchan * sizeof(FixedCarry), hipMemcpyHostToDevice, S));
    }
    if (seeds) HIP_TRY(hipMemcpyAsync(d_seeds, seeds, n * sizeof(double), hipMemcpyHostToDevice, S));
    const bool chained = reference && !seeds;
    // where a block's descriptor takes its carrier phase from: Prep::est (32-byte rows, the double at offset 8), or the caller's states
    const char *est_rows = seeds ? reinterpret_cast<const char *>(d_seeds) : reinterpret_cast<const char *>(d_prep) + 8;
    const int est_stride = seeds ? 8 : 32;
    PackJob pj = {ch, h_chan, nullptr, nchan, delt, 0, 0, 0};
    hipError_t he = hipSuccess;
    char err[400] = "";
    SynthClass cls;                                         // of the pieces staged so far
    double t_first_launch = 0.0;
    int timed_blocks = 0;
    Event *staged = e.evaluated;                            // [k]: piece k's descriptors are in the set (and a snapshot of the control block behind them)
    for (int k = 0; k < npieces && rc == GPSIQ_OK; ++k) {
        const int b0 = k ? ends[k - 1] : 0, nb = ends[k] - b0;
        const size_t off = (size_t) b0 * nchan, cnt = (size_t) nb * nchan;
        if (kind == kSrcDevice) he = launch_pack_raw(static_cast<const gpsiq_chan_t *>(dev_src) + off, nb, nchan, delt, d_chan + off, d_ctrl, S);
        else if (kind == kSrcPinned) {
            he = hipMemcpyAsync(d_raw + off, ch + off, cnt * sizeof(gpsiq_chan_t), hipMemcpyHostToDevice, S);
            if (he == hipSuccess) he = launch_pack_raw(d_raw + off, nb, nchan, delt, d_chan + off, d_ctrl, S);
        } else {
            const double tp = gpsiq_wall_ms();
            PackJob part = pj;
            part.ch = ch + off; part.out = h_chan + off;
            pack_host(&part, nb);
            pj.mx = part.mx > pj.mx ? part.mx : pj.mx; pj.max_active = part.max_active > pj.max_active ? part.max_active : pj.max_active;
            pj.max_amp = part.max_amp > pj.max_amp ? part.max_amp : pj.max_amp;
            e.host_ms += gpsiq_wall_ms() - tp; host_part[0] += gpsiq_wall_ms() - tp;
            he = hipMemcpyAsync(d_chan + off, h_chan + off, cnt * sizeof(ev::DChan), hipMemcpyHostToDevice, S);
        }
        if (he == hipSuccess && chained)
            he = launch_chain(d_chan + off, (int) sizeof(ev::DChan), nb, nchan, delt, nsamp, k ? d_est + (size_t) k * GPSIQ_MAX_CHAN : nullptr, 0,
                              d_prep + off * c->chain.kPrepBytes, d_c_before + (size_t) k * GPSIQ_MAX_CHAN,
                              d_est + (size_t) (k + 1) * GPSIQ_MAX_CHAN, d_maps + off, S, 1);
        if (he == hipSuccess) {
            if (reference) he = launch_quantize_est(d_chan, b0, nb, nchan, delt, nsamp, est_rows, est_stride, d_set, d_ctrl, S);
            else he = launch_quantize_fixed(d_chan, b0, nb, nchan, delt, nsamp, d_set, d_fix, d_ctrl, S);
        }
        if (he == hipSuccess && kind != kSrcPageable) he = hipMemcpyAsync(&h_ctrl[k], d_ctrl, sizeof(EvalCtrl), hipMemcpyDeviceToHost, S);
        if (he == hipSuccess) he = hipEventRecord(staged[k].get(), S);
        // the launch parameters of the synthesis kernel: from the pool's pack at once, from the device's pack behind the event
        if (he == hipSuccess && kind != kSrcPageable) he = hipEventSynchronize(staged[k].get());
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, piece %d: %s", k, hipGetErrorString(he)); break; }
        if (kind == kSrcPageable) cls = {pj.mx, std::max(pj.max_active, 1), pj.max_amp};
        else {
            const EvalCtrl &ck = h_ctrl[k];
            cls = {std::max<uint64_t>(cls.max_code_step, ck.max_code_step), std::max({cls.max_active, ck.max_active, 1}), std::max<long>(cls.max_amplitude, (long) ck.max_amp)};
        }
        hipStream_t s = gpsiq_piece_stream(c, k);
        he = hipStreamWaitEvent(s, staged[k].get(), 0);
        if (he == hipSuccess) {
            // the last piece's synthesis is timed: the rate the piece sizes are planned with is a measured one (gpsiq_note_kernel_rate)
            if (k == npieces - 1) (void) hipEventRecord(e.t_synth0.get(), s);
            he = launch_variant(auto_variant(cls.max_code_step), d_set, nchan, nsamp, sample_size, out.target(b0), out.stride, b0, nb, d_tab, s, cls, nullptr,
                                gpsiq_noise_at(c, c->call_block));
            if (k == npieces - 1) { (void) hipEventRecord(e.t_synth1.get(), s); timed_blocks = nb; }
            if (trace && k == 0) t_first_launch = gpsiq_wall_ms() - t0;
        }
        // a piece crosses to the destination as soon as it is rendered (the next piece's kernel covers the copy); in
        // GPSIQ_NCO_REFERENCE the few blocks that hold a patched sample are copied once more behind apply_patches
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, piece %d launch: %s", k, hipGetErrorString(he)); }
        else if (out.rendered(b0, nb, s) != GPSIQ_OK) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, piece %d launch: %s", k, gpsiq_last_error()); }
    }
    const double t_queued = gpsiq_wall_ms();

    // ---- phase B (GPSIQ_NCO_REFERENCE): the chain behind the descriptors, repair, the evaluation ---------------------------------
    // One launch each over the WHOLE timeline, whatever the synthesis pieces were: every launch of the chain has a latency floor
    // (a wave's walk, ~0.1 ms), and this path has to be through before the synthesis is (three pieces of 2 000 blocks: 2.03 ms per
    // call against 1.84 with one).
    bool host_owned[GPSIQ_MAX_CHAN] = {};
    double host_end[GPSIQ_MAX_CHAN] = {};
    int host_last_prn[GPSIQ_MAX_CHAN] = {};
    const std::vector<int> chain_ends(1, nblocks);
    const int nchain = 1;
    if (rc == GPSIQ_OK && chained) {
        int max_seg = 32;
        if (const char *sv = std::getenv("GPSIQ_CHAIN_STRETCHES")) { const int v = std::atoi(sv); if (v >= 1 && v <= 32) max_seg = v; }
        for (int k = 0; k < nchain && he == hipSuccess; ++k) {
            const int b0 = k ? chain_ends[k - 1] : 0, nb = chain_ends[k] - b0;
            const size_t off = (size_t) b0 * nchan;
            he = launch_chain(d_chan + off, (int) sizeof(ev::DChan), nb, nchan, delt, nsamp, nullptr, max_seg, d_prep + off * c->chain.kPrepBytes,
                              d_c_before + (size_t) k * GPSIQ_MAX_CHAN, nullptr, d_maps + off, S, 2);
#ifdef GPSIQ_TEST_HOOKS          // fault injection (tests/test_gpu_verify.py builds a library with it): one map made wrong without making it unusable
            if (he == hipSuccess) he = launch_test_corrupt_map(d_maps, b0, nb, nchan, S);
#endif
            if (he == hipSuccess) he = launch_link_scan(d_chan, d_maps, b0, nb, nchan, delt, d_link, d_ctrl, k, S);
            if (he == hipSuccess) he = hipMemcpyAsync(&h_ctrl[k], d_ctrl, sizeof(EvalCtrl), hipMemcpyDeviceToHost, S);
            if (he == hipSuccess) he = hipEventRecord(e.linked[k].get(), S);
        }
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, chain: %s", hipGetErrorString(he)); }
    }
    for (int k = 0; k < nchain && rc == GPSIQ_OK && reference; ++k) {
        const int b0 = k ? chain_ends[k - 1] : 0, nb = chain_ends[k] - b0;
        if (chained) {
            he = hipEventSynchronize(e.linked[k].get());
            if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, piece %d: %s", k, hipGetErrorString(he)); break; }
            const EvalCtrl &ck = h_ctrl[k];
            bool need = false;
            for (int i = 0; i < nchan; ++i) need = need || ck.unknown[k][i] > 0 || host_owned[i];
            if (need) {
                // A block whose certified map does not apply (a slow block, a sign change, a range the estimate missed): the host
                // walker takes that slot from this piece on -- the slot's column of maps and rows comes back, it is linked / walked from
                // the state it enters the piece with (lane::link_block + the true walk, as rounds 4-5 did for every slot), and its
                // start states go back up before the piece is evaluated.  The device's own scan goes on for the other slots, and
                // the synthesis is not held up: it runs from the estimates.
                const double tr = gpsiq_wall_ms();
                const int lead = b0 > 0 ? 1 : 0;                                   // the row before the piece too: which satellite the slot had
                if (e.reserve_repair((size_t) nb + 1) != GPSIQ_OK) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, repair buffers: %.300s", gpsiq_last_error()); break; }
                EvalSlotRow *const d_slot = e.d_slot.get(), *const h_slot = e.h_slot.get();
                double *const d_col = e.d_col.get(), *const h_col = e.h_col.get();
                for (int i = 0; i < nchan && rc == GPSIQ_OK; ++i) {
                    if (!(ck.unknown[k][i] > 0 || host_owned[i])) continue;
                    // the slot's column (map + chain inputs + the starts the scan wrote), one small copy instead of every slot's rows
                    he = launch_gather_slot(d_chan, d_maps, b0 - lead, nb + lead, nchan, i, d_slot, E);
                    if (he == hipSuccess) he = hipMemcpyAsync(h_slot, d_slot, (size_t) (nb + lead) * sizeof(EvalSlotRow), hipMemcpyDeviceToHost, E);
                    if (he == hipSuccess) he = hipStreamSynchronize(E);
                    if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, repair: %s", hipGetErrorString(he)); break; }
                    if (!host_owned[i]) {
                        // the state the slot enters the piece with: the scan knew every start up to its first block that does not link
                        host_last_prn[i] = lead && h_slot[0].prn > 0 ? h_slot[0].prn : 0;
                        host_end[i] = h_slot[lead].start;
                    }
                    long linked = 0, walked = 0;
                    int bad = -1;
                    if (!link_slot_host(h_slot + lead, b0, b0 + nb, delt, nsamp, &host_end[i], &host_last_prn[i], h_col, &linked, &walked, &bad)) {
                        rc = GPSIQ_E_RANGE; std::snprintf(err, sizeof err, "block %d: carrier phase or Doppler outside the NCO format", bad);
                        break;
                    }
                    chain_count(linked, walked);
                    he = hipMemcpyAsync(d_col, h_col, (size_t) nb * sizeof(double), hipMemcpyHostToDevice, E);
                    if (he == hipSuccess) he = launch_scatter_starts(d_chan, b0, nb, nchan, i, d_col, E);
                    if (he == hipSuccess) he = hipStreamSynchronize(E);                   // (the staging is reused for the next slot)
                    if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, repair upload: %s", hipGetErrorString(he)); break; }
                    if (!host_owned[i]) { host_owned[i] = true; ++e.last_repaired; }
                }
                e.host_ms += gpsiq_wall_ms() - tr; host_part[1] += gpsiq_wall_ms() - tr;
                if (rc != GPSIQ_OK) break;
            }
        }
        he = hipStreamWaitEvent(E, chained ? e.linked[k].get() : staged[npieces - 1].get(), 0);
        if (he == hipSuccess)
            he = launch_eval(d_chan, b0, nb, nchan, delt, nsamp, d_tab, est_rows, est_stride, d_patches, list_cap(kPatchCap), d_host, list_cap(kHostCap), d_ctrl,
                             seeds ? d_seeds : nullptr, E);
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, piece %d evaluation: %s", k, hipGetErrorString(he)); }
    }

    // ---- the end of the evaluation: errors, the host walker's share, the patches -----------------------------------------------
    EvalCtrl &fin = h_ctrl[kEvalMaxPieces];
    fin = zero;
    size_t npatch_total = 0;
    bool fall_back = false;
    if (rc == GPSIQ_OK) {
        // (the fixed model's kernels ran on the staging stream: the results' way back waits for the last piece's)
        he = hipStreamWaitEvent(E, staged[npieces - 1].get(), 0);
        if (he == hipSuccess) he = hipMemcpyAsync(&fin, d_ctrl, sizeof(EvalCtrl), hipMemcpyDeviceToHost, E);
        if (he == hipSuccess && reference) {
            // the first entries of both lists ride along (nearly always all there are)
            he = hipMemcpyAsync(h_patches, d_patches, 1024 * sizeof(gpsiq_patch_t), hipMemcpyDeviceToHost, E);
            if (he == hipSuccess) he = hipMemcpyAsync(h_host, d_host, 256 * sizeof(EvalHostItem), hipMemcpyDeviceToHost, E);
            if (he == hipSuccess && !seeds) he = hipMemcpyAsync(h_link, d_link, (size_t) nchan * sizeof(LinkCarry), hipMemcpyDeviceToHost, E);
        }
        if (he == hipSuccess && !reference) he = hipMemcpyAsync(h_fix, d_fix, (size_t) nchan * sizeof(FixedCarry), hipMemcpyDeviceToHost, E);
        if (he == hipSuccess) he = hipStreamSynchronize(E);
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, results: %s", hipGetErrorString(he)); }
    }
    if (rc == GPSIQ_OK && fin.err_key != ~0ull) {
        // the descriptor the device quantiser refused, in the host quantiser's words
        const size_t flat = (size_t) (fin.err_key >> 8);
        const int status = (int) (fin.err_key & 0xff);
        gpsiq_chan_t bad;
        if (kind == kSrcDevice) (void) hipMemcpy(&bad, ch + flat, sizeof bad, hipMemcpyDeviceToHost);
        else bad = ch[flat];
        gpsiq_qchan_t tmp;
        if (status == ev::kQStart) {
            rc = GPSIQ_E_RANGE;
            std::snprintf(err, sizeof err, "block %d: prn %d: start phase outside [0, 1]", (int) (flat / nchan), bad.prn);
        } else {
            if (reference && !(bad.carr_phase >= 0.0 && bad.carr_phase < 1.0)) bad.carr_phase = 0.0;       // (not the evaluation's business: eval_block)
            const int qrc = quantize_one(bad, delt, nsamp, nullptr, &tmp, nullptr);
            rc = qrc != GPSIQ_OK ? qrc : ev::qstatus_code(status);
            if (qrc != GPSIQ_OK) std::snprintf(err, sizeof err, "block %d: %.280s", (int) (flat / nchan), gpsiq_last_error());
            else std::snprintf(err, sizeof err, "block %d: descriptor refused by the device quantiser (status %d)", (int) (flat / nchan), status);
        }
    }
    std::vector<gpsiq_patch_t> patches;
    if (rc == GPSIQ_OK && reference) {
        if (fin.npatch > list_cap(kPatchCap) || fin.nhost > list_cap(kHostCap)) fall_back = true;       // more than the lists hold (a rate far outside the design range)
        else {
            if (fin.npatch > 1024) he = hipMemcpy(h_patches + 1024, d_patches + 1024, (size_t) (fin.npatch - 1024) * sizeof(gpsiq_patch_t), hipMemcpyDeviceToHost);
            if (he == hipSuccess && fin.nhost > 256) he = hipMemcpy(h_host + 256, d_host + 256, (size_t) (fin.nhost - 256) * sizeof(EvalHostItem), hipMemcpyDeviceToHost);
            if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, lists: %s", hipGetErrorString(he)); }
        }
        if (rc == GPSIQ_OK && !fall_back) {
            const double th = gpsiq_wall_ms();
            patches.assign(h_patches, h_patches + fin.npatch);
            if (fin.nhost) {
                // what the device left to the host walker: those channels' patches from eval_block, in place of whatever the device
                // had emitted for them before it gave up
                std::vector<uint64_t> keys;
                for (unsigned k = 0; k < fin.nhost; ++k) keys.push_back((uint64_t) h_host[k].block << 8 | h_host[k].slot);
                std::sort(keys.begin(), keys.end());
                patches.erase(std::remove_if(patches.begin(), patches.end(), [&](const gpsiq_patch_t &p) {
                    return std::binary_search(keys.begin(), keys.end(), (uint64_t) p.block << 8 | p.slot); }), patches.end());
                // (descriptors that lie in device memory: the few the walker needs come back in one go)
                if (kind == kSrcDevice) {
                    he = fin.nhost > e.h_items.cap() ? e.h_items.reserve((size_t) fin.nhost + 64) : hipSuccess;
                    for (unsigned k = 0; k < fin.nhost && he == hipSuccess; ++k)
                        he = hipMemcpyAsync(&e.h_items[k], ch + (size_t) h_host[k].block * nchan + h_host[k].chan, sizeof(gpsiq_chan_t), hipMemcpyDeviceToHost, E);
                    if (he == hipSuccess) he = hipStreamSynchronize(E);
                    if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, descriptors for the host walker: %s", hipGetErrorString(he)); }
                }
                if (rc == GPSIQ_OK) {
                    // (one walk of a block's samples each, ~0.1 ms: side by side on the pool, the lists joined in the items' order)
                    struct WJob { const EvalHostItem *items; const gpsiq_chan_t *own, *all; int nchan, nsamp; double delt; std::vector<gpsiq_patch_t> *out; int *rcs; std::array<char, 300> *texts; };
                    std::vector<std::vector<gpsiq_patch_t>> found(fin.nhost);
                    std::vector<int> rcs(fin.nhost, GPSIQ_OK);
                    std::vector<std::array<char, 300>> texts(fin.nhost);
                    WJob wj = {h_host, kind == kSrcDevice ? e.h_items.get() : nullptr, ch, nchan, nsamp, delt, found.data(), rcs.data(), texts.data()};
                    parallel_for((int) fin.nhost, 0, 1, [](void *p, int k0, int k1) {
                        WJob &j = *static_cast<WJob *>(p);
                        for (int k = k0; k < k1; ++k) {
                            const EvalHostItem &h = j.items[k];
                            const gpsiq_chan_t &one = j.own ? j.own[k] : j.all[(size_t) h.block * j.nchan + h.chan];
                            gpsiq_qchan_t q;
                            j.rcs[k] = eval_block_host(one, h.start, &h.seed, j.delt, j.nsamp, (int) h.block, (int) h.slot, &q, &j.out[k]);
                            if (j.rcs[k] != GPSIQ_OK) std::snprintf(j.texts[k].data(), j.texts[k].size(), "block %u: %.280s", h.block, gpsiq_last_error());
                        }
                    }, &wj);
                    for (unsigned k = 0; k < fin.nhost; ++k) {
                        if (rcs[k] != GPSIQ_OK && rc == GPSIQ_OK) { rc = rcs[k]; std::snprintf(err, sizeof err, "%s", texts[k].data()); }
                        patches.insert(patches.end(), found[k].begin(), found[k].end());
                    }
                }
            }
            std::sort(patches.begin(), patches.end(), patch_before);
            npatch_total = patches.size();
            e.host_ms += gpsiq_wall_ms() - th; host_part[2] += gpsiq_wall_ms() - th;
        }
    }
    // the patches go behind the synthesis of every piece: join the two piece streams on the first
    if (rc == GPSIQ_OK && reference && !fall_back) {
        he = hipSuccess;
        if (npieces > 1) { he = hipEventRecord(e.joined.get(), c->stream2.get()); if (he == hipSuccess) he = hipStreamWaitEvent(c->stream.get(), e.joined.get(), 0); }
        if (he == hipSuccess && npatch_total) {
            he = nb_.d_patch.reserve(gpsiq_patch_room(npatch_total));
            if (he == hipSuccess) {
                std::memcpy(h_patches, patches.data(), npatch_total * sizeof(gpsiq_patch_t));
                he = hipMemcpyAsync(nb_.d_patch.get(), h_patches, npatch_total * sizeof(gpsiq_patch_t), hipMemcpyHostToDevice, c->stream.get());
            }
            if (he == hipSuccess) he = launch_patches(d_set, nchan, nsamp, sample_size, out.target(0), out.stride, 0, nblocks, d_tab, nb_.d_patch.get(), (int) npatch_total,
                                                       c->stream.get(), gpsiq_noise_at(c, c->call_block));
        }
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, patches: %s", hipGetErrorString(he)); }
        else if (out.again(c->stream.get(), patches) != GPSIQ_OK) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, patches: %s", gpsiq_last_error()); }
    }

    // ---- GPSIQ_CHAIN_VERIFY=N: every N-th block that went through its certified map is also walked serially ---------------------
    // (on a few host threads, from the start state the scan gave it, when everything of the call has been queued and only the
    // synthesis is still running: gps.c:2821-2826 is the judge)
    const int verify_n = reference && !seeds ? chain_verify_every() : 0;
    unsigned verified = 0;
    if (rc == GPSIQ_OK && verify_n > 0) {
        const double tv = gpsiq_wall_ms();
        he = hipMemcpyAsync(h_chan, d_chan, n * sizeof(ev::DChan), hipMemcpyDeviceToHost, E);
        if (he == hipSuccess) he = hipMemcpyAsync(h_link, d_link, (size_t) nchan * sizeof(LinkCarry), hipMemcpyDeviceToHost, E);
        if (he == hipSuccess) he = hipStreamSynchronize(E);
        if (he != hipSuccess) { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation, verify: %s", hipGetErrorString(he)); }
        else {
            struct VJob { const ev::DChan *ch; const LinkCarry *end; const bool *skip; int nblocks, nchan, nsamp, every; double delt; long bad; unsigned count; };
            VJob vj = {h_chan, h_link, host_owned, nblocks, nchan, nsamp, verify_n, delt, -1, 0};
            parallel_for(nblocks, 4, 64, [](void *p, int b0, int b1) {
                VJob &j = *static_cast<VJob *>(p);
                unsigned count = 0;
                for (int b = b0; b < b1; ++b)
                    for (int i = 0; i < j.nchan; ++i) {
                        if ((b + i) % j.every || j.skip[i]) continue;
                        const ev::DChan &d = j.ch[(size_t) b * j.nchan + i];
                        if (d.prn <= 0 || !(d.start >= 0.0 && d.start <= 1.0) || !(std::fabs(d.f_carr * j.delt) < 0.5)) continue;
                        double want;
                        if (b + 1 < j.nblocks) {
                            const ev::DChan &nx = j.ch[(size_t) (b + 1) * j.nchan + i];
                            if (nx.prn != d.prn) continue;                       // the slot ends or is re-seeded: nobody reads this block's end
                            want = nx.start;
                        } else if (j.end[i].known) want = j.end[i].y;
                        else continue;
                        const double got = chain_block_true(d.f_carr, j.delt, j.nsamp, d.start);
                        ++count;
                        if (bits_of(got) != bits_of(want)) __sync_val_compare_and_swap(&j.bad, -1L, (long) b * j.nchan + i);
                    }
                __sync_fetch_and_add(&j.count, count);
            }, &vj);
            verified = vj.count;
            if (vj.bad >= 0) {
                rc = GPSIQ_E_VERIFY;
                std::snprintf(err, sizeof err, "block %ld slot %ld: the state after the block through its certified map is not the serial walk's (GPSIQ_CHAIN_VERIFY=%d)",
                              vj.bad / nchan, vj.bad % nchan, verify_n);
            }
        }
        e.host_ms += gpsiq_wall_ms() - tv;
    }

    // ---- drain: on every path nothing may still be writing the caller's buffer or reading our staging -------------------------
    const double t_drain = gpsiq_wall_ms();
    const hipError_t d0 = hipStreamSynchronize(S), d1 = hipStreamSynchronize(E);
    if (rc == GPSIQ_OK && (d0 != hipSuccess || d1 != hipSuccess))
        { rc = GPSIQ_E_DEVICE; std::snprintf(err, sizeof err, "device evaluation: %s", hipGetErrorString(d0 != hipSuccess ? d0 : d1)); }
    rc = out.finish("device evaluation", rc != GPSIQ_OK ? fail(rc, "%s", err) : GPSIQ_OK);     // (after an error: drains, the error stands)
    if (rc != GPSIQ_OK) return rc;
    if (timed_blocks > 0) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e.t_synth0.get(), e.t_synth1.get()) == hipSuccess && ms > 0.02f)
            gpsiq_note_kernel_rate((double) timed_blocks * (double) nsamp * (double) nchan / (ms * 1e-3));
    }
    if (fall_back) {
        // the lists overflowed: not handled after all -- the caller's host path does the whole call again (dst is rewritten), from
        // descriptors the host can read
        __atomic_fetch_add(&g_evd_stats[5], 1, __ATOMIC_RELAXED);
        *handled = 0;
        return GPSIQ_OK;
    }

    // ---- the resident set and the carried state ------------------------------------------------------------------------------
    c->cur = next;
    c->d_desc = d_set;
    c->nblocks = nblocks; c->nchan = nchan; c->cls = cls;
    nb_.npatch = (int) npatch_total;
    nb_.active_per_block.assign((size_t) nblocks, (uint8_t) nchan);
    nb_.upload_pending = false;
    if (reference) {
        if (carr_phase_out && !seeds)
            for (int i = 0; i < nchan; ++i) {
                if (host_owned[i]) carr_phase_out[i] = host_last_prn[i] ? host_end[i] : last[i].carr_phase;
                else carr_phase_out[i] = h_link[i].prn > 0 ? h_link[i].y : last[i].carr_phase;
            }
        chain_count((long) fin.linked, 0);
    } else {
        for (int i = 0; i < nchan; ++i) gpsiq_hand_back(c, i, h_fix[i].prn, h_fix[i].phase, carr_phase_out);
    }
    e.last_nhost = fin.nhost; e.last_npatch = (unsigned) npatch_total;
    __atomic_fetch_add(&g_evd_stats[1], (uint64_t) n, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_evd_stats[2], (uint64_t) fin.nhost, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_evd_stats[3], (uint64_t) e.last_repaired, __ATOMIC_RELAXED);
    __atomic_fetch_add(&g_evd_stats[4], (uint64_t) npatch_total, __ATOMIC_RELAXED);
    if (trace)
        std::fprintf(stderr, "[gpsiq trace] device evaluation (%s, descriptors %s), %d blocks in %d pieces (head %d): queued by %.3f ms, first synthesis launched at %.3f ms, "
                             "draining from %.3f ms, whole call %.3f ms; host stages %.3f ms (pack %.3f, repair %.3f, lists + walker %.3f); %u patches, %u channels to the host walker, %u slots repaired, %u blocks verified\n",
                     reference ? "reference NCO" : "fixed-point NCO", kind == kSrcDevice ? "in device memory" : kind == kSrcPinned ? "page-locked" : "pageable (packed by the pool)",
                     nblocks, npieces, ends[0], t_queued - t0, t_first_launch, t_drain - t0, gpsiq_wall_ms() - t0, e.host_ms, host_part[0], host_part[1], host_part[2], (unsigned) npatch_total, fin.nhost, e.last_repaired, verified);
    return GPSIQ_OK;
}
