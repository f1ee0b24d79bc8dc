// gpsiq_batch.cpp -- the drop-in calls of one context (include/gpsiq.h: gpsiq_generate_block[_async], gpsiq_wait,
// gpsiq_generate_quantized, gpsiq_generate_batch; gpsiq_generate_seeded): the output of a batch call (PieceOut), the host path of
// GPSIQ_NCO_REFERENCE with the carrier chain's device launches, the measured kernel rate.  HIP runtime only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gpsiq_calls.h"
#include "gpsiq_ctx.h"

using namespace gpsiq;

// ---- the output of a batch call (PieceOut, gpsiq_ctx.h) ----------------------------------------------------------------------

int PieceOut::begin(gpsiq_ctx *ctx, int nblocks_, int nsamp, int sample_size, void *dst_, int dst_is_device_)
{
    c = ctx; nblocks = nblocks_; copies = 0; dst = static_cast<uint8_t *>(dst_); dst_is_device = dst_is_device_ != 0;
    blk_bytes = block_bytes(nsamp, sample_size); stride = block_stride(nsamp, sample_size);
    direct = dst_is_device && stride == blk_bytes && !((uintptr_t) dst & 3);
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = stride * (size_t) nblocks;
    if (!direct) HIP_TRY(c->d_out.reserve(bytes));            // (sized before anything is queued)
    return GPSIQ_OK;
}

// blocks [b0, b0 + nb) from the staging to dst on stream s: one linear copy where the rows are contiguous
static hipError_t copy_rows(const PieceOut &o, int b0, int nb, hipStream_t s)
{
    const hipMemcpyKind kind = o.dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    uint8_t *to = o.dst + (size_t) b0 * o.blk_bytes;
    if (o.stride == o.blk_bytes) return hipMemcpyAsync(to, o.target(b0), o.blk_bytes * (size_t) nb, kind, s);
    return hipMemcpy2DAsync(to, o.blk_bytes, o.target(b0), o.stride, o.blk_bytes, (size_t) nb, kind, s);
}

// the copy of piece k goes on copy_stream[k & 1] (consecutive copies queue back to back) once the piece's kernel has finished
int PieceOut::rendered(int b0, int nb, hipStream_t s)
{
    if (direct) return GPSIQ_OK;
    const int k = copies++ & 1;
    hipError_t e = hipEventRecord(c->chunk_done[k].get(), s);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->copy_stream[k].get(), c->chunk_done[k].get(), 0);
    if (e == hipSuccess) e = copy_rows(*this, b0, nb, c->copy_stream[k].get());
    return e == hipSuccess ? GPSIQ_OK : fail(GPSIQ_E_DEVICE, "piece copy: %s", hipGetErrorString(e));
}

int PieceOut::whole(hipStream_t s)
{
    if (direct) return GPSIQ_OK;
    const hipError_t e = copy_rows(*this, 0, nblocks, s);
    return e == hipSuccess ? GPSIQ_OK : fail(GPSIQ_E_DEVICE, "copy: %s", hipGetErrorString(e));
}

// behind the pieces' own copies, which may still be on their way (the copy streams are joined to s): every block that holds a
// patched sample, or the whole timeline when that is more than a quarter of it
int PieceOut::again(hipStream_t s, const std::vector<gpsiq_patch_t> &patches)
{
    if (direct || patches.empty()) return GPSIQ_OK;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = hipEventRecord(c->chunk_done[k].get(), c->copy_stream[k].get());
        if (e == hipSuccess) e = hipStreamWaitEvent(s, c->chunk_done[k].get(), 0);
    }
    size_t touched = 0;
    for (size_t k = 0; k < patches.size(); ++k) touched += k == 0 || patches[k].block != patches[k - 1].block;
    const hipMemcpyKind kind = dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (e == hipSuccess && touched * 4 > (size_t) nblocks) e = copy_rows(*this, 0, nblocks, s);
    else
        for (size_t k = 0; k < patches.size() && e == hipSuccess; ++k)
            if (k == 0 || patches[k].block != patches[k - 1].block)
                e = hipMemcpyAsync(dst + (size_t) patches[k].block * blk_bytes, target((int) patches[k].block), blk_bytes, kind, s);
    return e == hipSuccess ? GPSIQ_OK : fail(GPSIQ_E_DEVICE, "patched blocks: %s", hipGetErrorString(e));
}

int PieceOut::finish(const char *label, int rc)
{
    if (!c) return rc;
    (void) hipSetDevice(c->device);
    hipError_t e = hipSuccess;
    for (hipStream_t s : {c->copy_stream[0].get(), c->copy_stream[1].get(), c->stream.get(), c->stream2.get()})
        { const hipError_t d = hipStreamSynchronize(s); if (e == hipSuccess) e = d; }
    // every launch waited for its set's upload on the device and has finished; a set that was staged but never launched on (an
    // error in between) may still be uploading: the upload stream is drained too before the flags are dropped
    const hipError_t u = hipStreamSynchronize(c->up_stream.get());
    if (e == hipSuccess && u == hipSuccess)
        for (auto &b : c->buf) b.upload_pending = false;
    if (rc != GPSIQ_OK) return rc;
    if (e != hipSuccess) return fail(GPSIQ_E_DEVICE, "%s: %s", label, hipGetErrorString(e));
    if (u != hipSuccess) return fail(GPSIQ_E_DEVICE, "%s: descriptor upload", label);
    return GPSIQ_OK;
}

// ---- synchronous drop-in entry points ---------------------------------------

// A host-destination batch goes in pieces of d2h_chunk_blocks: kernel on c->stream, the copy of piece k behind it
// (PieceOut::rendered).  A device destination, or one piece: one kernel, then one copy.
// (nbase: absolute block index of q[0], for the receiver noise)
int gpsiq_run_to_host_or_device(gpsiq_ctx *c, const gpsiq_qchan_t *q, int nblocks, int nchan, int nsamp, int sample_size, void *dst,
                                int dst_is_device, uint64_t nbase)
{
    int rc = gpsiq_set_descriptors(c, q, nblocks, nchan);
    if (rc) return rc;
    if (!nblocks || !nsamp) return GPSIQ_OK;
    PieceOut out;
    rc = out.begin(c, nblocks, nsamp, sample_size, dst, dst_is_device);
    const int chunk = d2h_chunk_blocks(out.stride, piece_blocks_env());
    if (dst_is_device || chunk <= 0 || nblocks <= chunk) {
        if (rc == GPSIQ_OK) rc = gpsiq_launch_abs(c, 0, nblocks, nsamp, sample_size, out.target(0), out.stride, c->stream.get(), kAuto, nbase);
        if (rc == GPSIQ_OK) rc = out.whole(c->stream.get());
    } else
        for (int b0 = 0; b0 < nblocks && rc == GPSIQ_OK; b0 += chunk) {
            const int nb = nblocks - b0 < chunk ? nblocks - b0 : chunk;
            rc = gpsiq_launch_abs(c, b0, nb, nsamp, sample_size, out.target(b0), out.stride, c->stream.get(), kAuto, nbase);
            if (rc == GPSIQ_OK) rc = out.rendered(b0, nb, c->stream.get());
        }
    return out.finish("batch pieces", rc);
}

int gpsiq_check_gen_args(const gpsiq_ctx *c, const void *ch, const void *dst, int nblocks, int nchan, int nsamp, double fs, int sample_size)
{
    if (!c || (!ch && nblocks) || (!dst && nblocks && nsamp)) return fail(GPSIQ_E_ARG, "null argument");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d", nblocks, nchan);
    if (nsamp < 0 || !(fs > 0.0)) return fail(GPSIQ_E_ARG, "bad nsamp %d / fs %g", nsamp, fs);
    if (sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad sample size %d", sample_size);
    return gpsiq_check_level(c, sample_size);
}

// ---- GPSIQ_NCO_REFERENCE: walk and render in pieces ------------------------------------------
// The carrier chain is serial in time on the host, the render is not: the timeline is cut into pieces (ref_chunk_blocks,
// piece_ends), and while the device renders (and copies out) piece k the host threads (RefWalk, gpsiq_refwalk.cpp: a chain task and
// an evaluation task per channel and piece, taken piece-major from the shared pool) are in the pieces behind it.
// gpsiq_generate_reference_host renders from the calling thread; gpsiq_generate_batch_multi (gpsiq_multi.cpp) gives every device a
// thread, fed through a queue.  gpsiq_ref_piece queues piece k of a range without waiting: blocks [b0, b0 + nb) of the range, whose
// descriptors q and patches (block indices relative to b0) are the piece's own.
int gpsiq_ref_piece(gpsiq_ctx *c, PieceOut &out, int k, const gpsiq_qchan_t *q, int b0, int nb, int nchan, int nsamp, int ss, uint64_t nbase,
                    const std::vector<gpsiq_patch_t> &patches)
{
    int rc = gpsiq_stage_descriptors(c, q, nb, nchan, patches.data(), (int) patches.size(), true);
    if (rc || !nb || !nsamp) return rc;
    hipStream_t s = gpsiq_piece_stream(c, k);
    rc = gpsiq_launch_abs(c, 0, nb, nsamp, ss, out.target(b0), out.stride, s, kAuto, nbase + (uint64_t) b0);
    return rc ? rc : out.rendered(b0, nb, s);
}

// The kernel's rate is MEASURED: every batch call that renders through the device evaluation times its last piece's synthesis
// with events and keeps a running mean in the context (gpsiq_evaldev.cpp); until the first such call, and for the host rate, the
// figures of MI355X + EPYC 9575F stand in.  GPSIQ_RATE_KERNEL (channel-samples per second, read per call) overrides both.
static std::atomic<double> g_rate_kernel_measured{0.0};        // a running mean over every context's calls (the placement rules have no context at hand)
double gpsiq_rate_kernel()
{
    if (const char *e = std::getenv("GPSIQ_RATE_KERNEL")) { const double v = std::atof(e); if (v > 1e9) return v; }
    const double m = g_rate_kernel_measured.load(std::memory_order_relaxed);
    return m > 0.0 ? m : 6.0e12;
}
static double rate_chain_us() { return 2.2; }      // microseconds per block and channel of the serial walk on one host thread

void gpsiq_note_kernel_rate(double channel_samples_per_s)
{
    if (!(channel_samples_per_s > 1e10 && channel_samples_per_s < 1e15)) return;
    const double old = g_rate_kernel_measured.load(std::memory_order_relaxed);
    g_rate_kernel_measured.store(old > 0.0 ? 0.75 * old + 0.25 * channel_samples_per_s : channel_samples_per_s, std::memory_order_relaxed);
}

// ---- the carrier chain on the device (its buffers, streams and events: gpsiq_ctx::Chain::reserve) ----------------------------
// Level 1 of the chain for blocks [b0, b0 + nb) of the inputs staged in c->chain.h_in, queued on the chain stream without
// waiting: upload, two kernels, the maps back into c->chain.h_maps (same rows), `landed` recorded behind them.  part 0 starts
// from `start` (host, may be null: the timeline begins here); part 1 continues where part 0's scan ended, on the device.
static int chain_queue(gpsiq_ctx *c, int part, int b0, int nb, int nchan, double fs, int nsamp, const gpsiq_chain_est_t *start, int max_stretches)
{
    gpsiq_ctx::Chain &k = c->chain;
    const size_t off = (size_t) b0 * (size_t) nchan, n = (size_t) nb * (size_t) nchan;
    if (max_stretches <= 0) {
        max_stretches = 32;
        if (const char *e = std::getenv("GPSIQ_CHAIN_STRETCHES")) { const int v = std::atoi(e); if (v >= 1 && v <= 32) max_stretches = v; }
    }
    HIP_TRY(hipMemcpyAsync(k.d_in.get() + off, k.h_in.get() + off, n * sizeof(gpsiq_chain_in_t), hipMemcpyHostToDevice, k.stream.get()));
    gpsiq_chain_est_t *d_est = k.d_est.get(), *h_est = k.h_est.get();
    const gpsiq_chain_est_t *d_start = nullptr;
    if (part == 1) d_start = d_est + GPSIQ_MAX_CHAN;
    else if (start) {
        std::memcpy(h_est, start, (size_t) nchan * sizeof(gpsiq_chain_est_t));
        HIP_TRY(hipMemcpyAsync(d_est, h_est, (size_t) nchan * sizeof(gpsiq_chain_est_t), hipMemcpyHostToDevice, k.stream.get()));
        d_start = d_est;
    }
    if (part == 0) HIP_TRY(hipEventRecord(k.t0.get(), k.stream.get()));
    HIP_TRY(launch_chain(k.d_in.get() + off, (int) sizeof(gpsiq_chain_in_t), nb, nchan, 1.0 / fs, nsamp, d_start, max_stretches, k.d_prep.get() + off * k.kPrepBytes,
                         k.d_c_before.get() + part * GPSIQ_MAX_CHAN, d_est + (part + 1) * GPSIQ_MAX_CHAN, k.d_maps.get() + off, k.stream.get()));
    HIP_TRY(hipEventRecord(k.t1.get(), k.stream.get()));
    // the maps' way back on a stream of its own: the next launch's kernels follow these at once (a callback queued between
    // them held the second launch up by ~0.1 ms)
    HIP_TRY(hipEventRecord(k.walked[part].get(), k.stream.get()));
    HIP_TRY(hipStreamWaitEvent(k.back.get(), k.walked[part].get(), 0));
    HIP_TRY(hipMemcpyAsync(k.h_maps.get() + off, k.d_maps.get() + off, n * sizeof(gpsiq_chain_map_t), hipMemcpyDeviceToHost, k.back.get()));
    HIP_TRY(hipMemcpyAsync(h_est + (part + 1) * GPSIQ_MAX_CHAN, d_est + (part + 1) * GPSIQ_MAX_CHAN, (size_t) nchan * sizeof(gpsiq_chain_est_t),
                           hipMemcpyDeviceToHost, k.back.get()));
    HIP_TRY(hipEventRecord(k.landed.get(), k.back.get()));
    return GPSIQ_OK;
}

static int chain_drain(gpsiq_ctx *c)
{
    const hipError_t a = hipStreamSynchronize(c->chain.stream.get()), b = hipStreamSynchronize(c->chain.back.get());
    if (a != hipSuccess || b != hipSuccess) return fail(GPSIQ_E_DEVICE, "carrier chain, level 1: %s", hipGetErrorString(a != hipSuccess ? a : b));
    return GPSIQ_OK;
}

// ... and waited for
int gpsiq_chain_maps_staged(gpsiq_ctx *c, int nblocks, int nchan, double fs, int nsamp, const gpsiq_chain_est_t *start, int max_stretches,
                            gpsiq_chain_est_t *end)
{
    gpsiq_ctx::Chain &k = c->chain;
    int rc = chain_queue(c, 0, 0, nblocks, nchan, fs, nsamp, start, max_stretches);
    if (rc) { (void) chain_drain(c); return rc; }
    rc = chain_drain(c);
    if (rc) return rc;
    (void) hipEventElapsedTime(&k.last_ms, k.t0.get(), k.t1.get());
    if (end) {
        std::memcpy(end, k.h_est.get() + GPSIQ_MAX_CHAN, (size_t) nchan * sizeof(gpsiq_chain_est_t));
        // f_carr is that of the last block in which the slot held a satellite, as gpsiq_chain_maps reports it.  The kernel hands on
        // the last block's: the same unless that block is unused -- then nothing on the device reads it (prn is 0), but a caller may
        for (int i = 0; i < nchan; ++i) {
            if (end[i].prn > 0) continue;
            double f = start ? start[i].f_carr : 0.0;
            for (int b = nblocks - 1; b >= 0; --b) {
                const gpsiq_chain_in_t &d = k.h_in.get()[(size_t) b * nchan + i];
                if (d.prn > 0) { f = d.f_carr; break; }
            }
            end[i].f_carr = f;
        }
    }
    return GPSIQ_OK;
}

int gpsiq_chain_maps_device(gpsiq_ctx_t *c, const gpsiq_chain_in_t *in, int nblocks, int nchan, double fs, int nsamp,
                            const gpsiq_chain_est_t *start, int max_stretches, gpsiq_chain_map_t *maps, gpsiq_chain_est_t *end, float *kernel_ms)
{
    if (!c || ((!in || !maps) && nblocks)) return fail(GPSIQ_E_ARG, "null argument");
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN || nsamp < 0 || !(fs > 0.0)) return fail(GPSIQ_E_ARG, "bad nblocks %d / nchan %d / nsamp %d / fs %g", nblocks, nchan, nsamp, fs);
    if (kernel_ms) *kernel_ms = 0.0f;
    if (nblocks == 0) return GPSIQ_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t) nblocks * (size_t) nchan;
    int rc = c->chain.reserve(n);
    if (rc) return rc;
    std::memcpy(c->chain.h_in.get(), in, n * sizeof(gpsiq_chain_in_t));
    rc = gpsiq_chain_maps_staged(c, nblocks, nchan, fs, nsamp, start, max_stretches, end);
    if (rc) return rc;
    std::memcpy(maps, c->chain.h_maps.get(), n * sizeof(gpsiq_chain_map_t));
    if (kernel_ms) *kernel_ms = c->chain.last_ms;
    return GPSIQ_OK;
}

// Whether a GPSIQ_NCO_REFERENCE batch walks level 1 of its carrier chain on the device.  The serial walk on host threads costs
// ~2.2 us per block and channel on each of min(threads, channels) threads and hides under the kernel of the piece before when
// the kernel is the slower side (25 Msps on sixteen threads); level 1 on the device costs a launch latency of ~0.25 ms before
// anything renders and nearly nothing after that.  GPSIQ_CHAIN=host / device decides by hand (read per call: A/B in one process).
bool gpsiq_chain_on_device(int nblocks, int nsamp, int nchan)
{
    const char *e = std::getenv("GPSIQ_CHAIN");
    if (e && !std::strcmp(e, "host")) return false;
    if (e && !std::strcmp(e, "device")) return nblocks > 1;
    if (nblocks < 48) return false;
    const int threads = host_threads() < nchan ? host_threads() : nchan;
    const double t_kernel = (double) nsamp * (double) nchan / gpsiq_rate_kernel();
    const double t_chain = rate_chain_us() * 1e-6 * (double) nchan / (double) (threads > 0 ? threads : 1);
    return t_chain > 0.5 * t_kernel;
}

// chain inputs of blocks [b0, b1) cut out of the descriptors into the page-locked staging: 296-byte descriptors, 24 bytes wanted
// of each -- memory-bound, so spread over the pool
void gpsiq_chain_stage_inputs(gpsiq_ctx *c, const gpsiq_chan_t *ch, int b0, int b1, int nchan)
{
    struct Job { const gpsiq_chan_t *ch; gpsiq_chain_in_t *out; } job = {ch + (size_t) b0 * nchan, c->chain.h_in.get() + (size_t) b0 * nchan};
    parallel_for((b1 - b0) * nchan, (b1 - b0) * nchan >= 8192 ? 0 : 1, 2048, [](void *p, int k0, int k1) {
        const Job &j = *static_cast<Job *>(p);
        gpsiq_chain_inputs(j.ch + k0, k1 - k0, j.out + k0);
    }, &job);
}

// ref_q / ref_start are kept between calls (a fresh 1.5 MB per call is four hundred page faults on the critical thread) -- but not
// at the size of the largest batch the context has ever seen: a call that needed less than an eighth of what is held (and what is
// held is more than 16 MB) gives the rest back
static void trim_retained(gpsiq_ctx *c, size_t need)
{
    if (c->ref_q.capacity() > (size_t) 8 * need && c->ref_q.capacity() * sizeof(gpsiq_qchan_t) > ((size_t) 16 << 20)) {
        std::vector<gpsiq_qchan_t>(need).swap(c->ref_q);
        std::vector<double>(c->ref_start.size() < need ? c->ref_start.size() : need).swap(c->ref_start);
    }
}

// GPSIQ_NCO_REFERENCE form of both drop-in calls: the carrier is the caller's double, walked exactly
int gpsiq_generate_reference_host(gpsiq_ctx *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs,
                                  int sample_size, void *dst, int dst_is_device, double *carr_phase_out, const double *seeds)
{
    const char *trace_env = std::getenv("GPSIQ_TRACE");
    const bool trace = trace_env != nullptr, trace_pieces = trace && std::atoi(trace_env) >= 2;      // GPSIQ_TRACE=2: every piece
    const double t0 = trace ? gpsiq_wall_ms() : 0.0;
    double t_wait = 0.0, t_queue = 0.0;
    size_t npatch = 0;
    std::vector<gpsiq_qchan_t> &q = c->ref_q;                // every element is written by its evaluation task before it is read
    if (q.size() < (size_t) nblocks * (size_t) nchan) q.resize((size_t) nblocks * (size_t) nchan);
    if (!seeds && c->ref_start.size() < (size_t) nblocks * (size_t) nchan) c->ref_start.resize((size_t) nblocks * (size_t) nchan);
    std::vector<gpsiq_patch_t> patches;
    PieceOut out;
    int rc = out.begin(c, nblocks, nsamp, sample_size, dst, dst_is_device);
    if (rc) return rc;
    const int chunk = ref_chunk_blocks(nblocks, nsamp, piece_blocks_env());
    std::vector<int> ends;
    const bool dev_chain = !seeds && gpsiq_chain_on_device(nblocks, nsamp, nchan);
    // (few growing pieces also with the chain on the device were tried: a 600-block piece is 0.3 ms of evaluation before it can
    // render, and the device waits for it: 2.6 ms per call against 2.4 at 2.6 Msps, profiles/r05_chain_ab.txt)
    piece_ends(0, nblocks, chunk, &ends, ref_kernel_bound(nsamp, nchan, gpsiq_rate_kernel(), host_threads()));
    // The carrier chain: level 1 (every block's certified map) on the device, parallel in time (gpsiq_chain_kernels.hip); the chain
    // tasks then link block to block through the maps.  Nothing renders before the first maps are back, and a launch is ~0.25 ms
    // however small: the timeline goes in two launches -- a head whose kernels cover the second launch, then the rest --, and the
    // walkers are let into the rest when its maps have landed (RefWalk::release_maps).
    double t_chain[3] = {};
    int head = nblocks;
    if (dev_chain) {
        rc = c->chain.reserve((size_t) nblocks * (size_t) nchan);
        if (rc) return rc;
        head = ref_head(ends, nblocks, nsamp, nchan, gpsiq_rate_kernel());
    }
    RefWalk w(ch, nblocks, nchan, 1.0 / fs, nsamp, q.data(), nullptr, nullptr, ends);
    w.seeds = seeds;                                         // start states known (gpsiq_generate_seeded): evaluation tasks only
    if (!seeds) w.start_out = c->ref_start.data();
    struct Landed { RefWalk *w; int upto; double *at, t0; };
    Landed landed[2] = {{&w, head, &t_chain[1], t0}, {&w, nblocks, &t_chain[2], t0}};
    // runs on a thread of the HIP runtime when the maps of a launch are in host memory: the walkers may link through them
    auto on_landed = [](void *p) {
        Landed *l = static_cast<Landed *>(p);
        if (l->t0 != 0.0) *l->at = gpsiq_wall_ms() - l->t0;
        l->w->release_maps(l->upto);
    };
    if (dev_chain) {
        w.in = c->chain.h_in.get(); w.maps = c->chain.h_maps.get(); w.maps_upto.store(0);
        gpsiq_chain_stage_inputs(c, ch, 0, head, nchan);
        rc = chain_queue(c, 0, 0, head, nchan, fs, nsamp, nullptr, 0);
        if (rc == GPSIQ_OK && hipLaunchHostFunc(c->chain.back.get(), on_landed, &landed[0]) != hipSuccess) rc = fail(GPSIQ_E_DEVICE, "hipLaunchHostFunc");
        if (rc == GPSIQ_OK && head < nblocks) {
            gpsiq_chain_stage_inputs(c, ch, head, nblocks, nchan);                               // under the head's kernels
            rc = chain_queue(c, 1, head, nblocks - head, nchan, fs, nsamp, nullptr, 0);
            if (rc == GPSIQ_OK && hipLaunchHostFunc(c->chain.back.get(), on_landed, &landed[1]) != hipSuccess) rc = fail(GPSIQ_E_DEVICE, "hipLaunchHostFunc");
        }
        if (rc) { (void) chain_drain(c); return rc; }
        if (trace) t_chain[0] = gpsiq_wall_ms() - t0;
    }
    // one piece (a block call, a short batch): walk here, then render; else the walk runs on the pool, driven by a helper
    // thread, and this thread renders every piece as soon as all channels are through it
    WalkThread walk(w, w.npieces() > 1);
    for (size_t k = 0; k < w.npieces() && rc == GPSIQ_OK; ++k) {
        const double tw = trace ? gpsiq_wall_ms() : 0.0;
        rc = w.wait_piece(k);
        if (rc != GPSIQ_OK) { (void) fail(rc, "%s", w.err); break; }
        const double tp = trace ? gpsiq_wall_ms() : 0.0;
        w.take_patches(k, &patches, true);
        npatch += patches.size();
        const int b0 = k ? w.ends[k - 1] : 0;
        rc = gpsiq_ref_piece(c, out, (int) k, q.data() + (size_t) b0 * nchan, b0, w.ends[k] - b0, nchan, nsamp, sample_size, c->call_block, patches);
        if (trace) {
            const double tq = gpsiq_wall_ms();
            t_wait += tp - tw; t_queue += tq - tp;
            if (trace_pieces)
                std::fprintf(stderr, "[gpsiq trace]   piece %zu, blocks [%d, %d): ready at %.3f ms, queued at %.3f ms, %zu patches\n",
                             k, b0, w.ends[k], tp - t0, tq - t0, patches.size());
        }
    }
    Status failed;
    failed.take(rc);
    if (!failed.ok()) w.abort();                             // nothing further is walked for a call that has failed
    if (dev_chain) {
        // the callbacks have run when the chain's streams have drained -- unless the device reported an error, in which case the
        // walkers must not be left waiting for maps that never land (and must not link through whatever h_maps held before)
        failed.take(chain_drain(c));
        if (!failed.ok()) w.abort();
        w.release_maps(nblocks);
    }
    walk.join();                                             // the walkers read ch and write q: never leave them running
    const double tf = trace ? gpsiq_wall_ms() : 0.0;
    const int frc = out.finish("reference NCO pieces");
    if (!failed.ok()) return failed.fail();
    if (w.rc != GPSIQ_OK) return fail(w.rc, "%s", w.err);
    if (frc != GPSIQ_OK) return frc;
    if (trace && dev_chain)
        std::fprintf(stderr, "[gpsiq trace] carrier chain, level 1 on the device: two launches queued by %.3f ms; the maps of the head (%d blocks) back at "
                             "%.3f ms, of the rest at %.3f ms\n", t_chain[0], head, t_chain[1], t_chain[2]);
    if (trace)
        std::fprintf(stderr, "[gpsiq trace] reference NCO, %d blocks in %zu pieces of %d: waited for the walkers %.2f ms (%zu patches), "
                             "validate + upload + launch %.2f ms, final wait %.2f ms, whole call %.2f ms\n",
                     nblocks, w.npieces(), chunk, t_wait, npatch, t_queue, gpsiq_wall_ms() - tf, gpsiq_wall_ms() - t0);
    if (carr_phase_out)
        for (int i = 0; i < nchan; ++i)
            carr_phase_out[i] = w.last_prn[i] ? w.carr_end[i] : ch[(size_t) (nblocks - 1) * nchan + i].carr_phase;
    trim_retained(c, (size_t) nblocks * (size_t) nchan);
    return GPSIQ_OK;
}

int gpsiq_generate_block_async(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nchan, int nsamp, double fs,
                               int sample_size, void *dst, double *carr_phase_out)
{
    if (!dst) return fail(GPSIQ_E_ARG, "null argument");
    int rc = gpsiq_check_gen_args(c, ch, dst, 1, nchan, nsamp, fs, sample_size);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const bool reference = c->nco_mode == GPSIQ_NCO_REFERENCE;
    gpsiq_qchan_t q[GPSIQ_MAX_CHAN];
    uint64_t next[GPSIQ_MAX_CHAN] = {};
    std::vector<gpsiq_patch_t> patches;
    double carr_end[GPSIQ_MAX_CHAN] = {};
    int last_prn[GPSIQ_MAX_CHAN] = {};
    const double delt = 1.0 / fs;
    if (reference) {
        // the carrier is the caller's double, walked exactly on the host: everything the device needs (start phases,
        // patches) and the phase to hand out are known before anything is queued
        rc = reference_timeline(ch, 1, nchan, delt, nsamp, q, &patches, carr_end, last_prn);
        if (rc) return rc;
    } else {
        for (int i = 0; i < nchan; ++i) {
            rc = quantize_one(ch[i], delt, nsamp, gpsiq_continues(c, i, ch[i]) ? &c->carry.phase[i] : nullptr, &q[i], &next[i]);
            if (rc) return rc;
        }
    }
    gpsiq_ctx::AsyncSlot &a = c->aslot[c->anext];
    if (a.busy) { HIP_TRY(hipEventSynchronize(a.done.get())); a.busy = false; }     // the ring is full: wait for its oldest block
    // each piece on its own: a call that failed half-way must not leave a slot that looks complete
    HIP_TRY(a.d.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(a.h.reserve(GPSIQ_MAX_CHAN));
    HIP_TRY(a.done.ensure());
    // compact (active channels first) and take the launch parameters, as gpsiq_set_descriptors does for a batch
    int na = 0;
    SynthClass cls;
    for (int i = 0; i < nchan; ++i) {
        if (!q[i].prn) continue;
        if (!(q[i].gain > -kMaxGain && q[i].gain < kMaxGain)) return fail(GPSIQ_E_RANGE, "gain %g outside the NCO format", q[i].gain);
        if (q[i].code_step > cls.max_code_step) cls.max_code_step = q[i].code_step;
        cls.max_amplitude += (long) (250.0 * std::fabs(q[i].gain));
        a.h[na++] = q[i];
    }
    for (int i = na; i < nchan; ++i) std::memset(&a.h[i], 0, sizeof(gpsiq_qchan_t));
    cls.max_active = na;
    const size_t blk_bytes = block_bytes(nsamp, sample_size), stride = block_stride(nsamp, sample_size);
    if (stride > a.out.cap()) HIP_TRY(a.out.reserve(stride ? stride : 16));
    if (!patches.empty()) {                                      // the slot is idle here (its event was waited for above)
        HIP_TRY(a.d_patch.reserve(gpsiq_patch_room(patches.size())));
        HIP_TRY(a.h_patch.reserve(gpsiq_patch_room(patches.size())));
    }
    if (nsamp > 0) {
        // once the first copy is queued a failure must not return with work in flight on the slot's page-locked staging (the next
        // call would rewrite it under the copy): the stream is drained first
        hipStream_t s = c->stream.get();
        hipError_t e = hipMemcpyAsync(a.d.get(), a.h.get(), (size_t) nchan * sizeof(gpsiq_qchan_t), hipMemcpyHostToDevice, s);
        const gpsiq::noise::Launch nz = gpsiq_noise_at(c, c->noise.next_block);
        if (e == hipSuccess) e = launch_variant(auto_variant(cls.max_code_step), a.d.get(), nchan, nsamp, sample_size, a.out.get(), stride, 0, 1, c->d_tab.get(), s, cls, nullptr, nz);
        if (e == hipSuccess && !patches.empty()) {
            std::memcpy(a.h_patch.get(), patches.data(), patches.size() * sizeof(gpsiq_patch_t));
            e = hipMemcpyAsync(a.d_patch.get(), a.h_patch.get(), patches.size() * sizeof(gpsiq_patch_t), hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = launch_patches(a.d.get(), nchan, nsamp, sample_size, a.out.get(), stride, 0, 1, c->d_tab.get(), a.d_patch.get(), (int) patches.size(), s, nz);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(dst, a.out.get(), blk_bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipEventRecord(a.done.get(), s);
        if (e != hipSuccess) {
            (void) hipStreamSynchronize(s);
            return fail(GPSIQ_E_DEVICE, "block: %s", hipGetErrorString(e));
        }
        a.busy = true;
        c->anext = (c->anext + 1) & 3;
    }
    ++c->noise.next_block;                                   // the block was rendered as absolute block next_block
    for (int i = 0; i < nchan; ++i) {
        if (!reference) gpsiq_hand_back(c, i, ch[i].prn > 0 ? ch[i].prn : 0, next[i], nullptr);
        const bool ours = reference ? last_prn[i] != 0 : ch[i].prn > 0;                  // else the caller's phase goes back as it came
        if (carr_phase_out) carr_phase_out[i] = !ours ? ch[i].carr_phase : reference ? carr_end[i] : c->carry.handed[i];
    }
    return GPSIQ_OK;
}

int gpsiq_generate_block(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nchan, int nsamp, double fs,
                         int sample_size, void *dst, double *carr_phase_out)
{
    if (!dst) return fail(GPSIQ_E_ARG, "null argument");
    int rc = gpsiq_check_gen_args(c, ch, dst, 1, nchan, nsamp, fs, sample_size);
    if (rc) return rc;
    // The asynchronous form -- descriptor upload, kernel (+ patches), copy into dst, all on the context's one stream -- and a
    // wait for THIS block: one host round trip where set_descriptors + launch + copy made two (84 -> ~60 us per block on MI355X).
    // Anything still queued by earlier _async calls completes first (same stream).  The continuation state goes back to what
    // it was if the device reports an error.
    const gpsiq_ctx::Carry carry0 = c->carry;
    const uint64_t next0 = c->noise.next_block;
    const int slot = c->anext;
    rc = gpsiq_generate_block_async(c, ch, nchan, nsamp, fs, sample_size, dst, carr_phase_out);
    if (rc) return rc;
    if (nsamp > 0) {
        gpsiq_ctx::AsyncSlot &a = c->aslot[slot];
        const hipError_t e = hipEventSynchronize(a.done.get());
        a.busy = false;
        if (e != hipSuccess) {
            c->carry = carry0;
            c->noise.next_block = next0;
            return fail(GPSIQ_E_DEVICE, "block: %s", hipGetErrorString(e));
        }
    }
    return GPSIQ_OK;
}

int gpsiq_wait(gpsiq_ctx_t *c)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    for (auto &a : c->aslot) a.busy = false;
    return GPSIQ_OK;
}

int gpsiq_generate_quantized(gpsiq_ctx_t *c, const gpsiq_qchan_t *q, int nblocks, int nchan, int nsamp,
                             int sample_size, void *dst, int dst_is_device)
{
    int rc = gpsiq_check_gen_args(c, q, dst, nblocks, nchan, nsamp, 1.0, sample_size);
    if (rc) return rc;
    if (nblocks == 0) return GPSIQ_OK;
    rc = gpsiq_run_to_host_or_device(c, q, nblocks, nchan, nsamp, sample_size, dst, dst_is_device, c->noise.next_block);
    if (rc == GPSIQ_OK) c->noise.next_block += (uint64_t) nblocks;
    return rc;
}

// ---- where the descriptors lie (gpsiq_ctx.h: SrcKind) -------------------------------------------------------------------------
int gpsiq_rows_kind(const gpsiq_ctx *c, const void *ch, const char *host_call, SrcKind *kind)
{
    SrcKind unused;
    if (!kind) kind = &unused;                            // (a call that only wants the refusal)
    *kind = kSrcPageable;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ch) != hipSuccess) { (void) hipGetLastError(); return GPSIQ_OK; }     // not the runtime's: the host's
    if (a.type == hipMemoryTypeHost) { *kind = kSrcPinned; return GPSIQ_OK; }
    if (a.type == hipMemoryTypeArray) return fail(GPSIQ_E_ARG, "descriptors in a HIP array: ch is linear memory");
    if (a.type != hipMemoryTypeDevice) return GPSIQ_OK;                  // unregistered, managed: read through the host
    if (host_call)
        return fail(GPSIQ_E_ARG, "%s: descriptors in device memory (device %d); this call reads ch on the host, pageable or page-locked", host_call, a.device);
    if (a.device != c->device)
        return fail(GPSIQ_E_ARG, "descriptors in device memory of device %d, the context is on device %d: ch is host memory or the context's device's",
                    a.device, c->device);
    *kind = kSrcDevice;
    return GPSIQ_OK;
}

// Descriptors in the context's device memory and the host path about to read them (the device path declined the batch, or its
// lists overflowed): the rows come down once, into page-locked staging the context keeps, and the call goes on with that pointer.
// (The path the device takes copies nothing but its two edge blocks.)
static int rows_to_host(gpsiq_ctx *c, const gpsiq_chan_t **ch, size_t n)
{
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(reserve_together(n, n + n / 4 + 16, c->h_rows));
    HIP_TRY(hipMemcpy(c->h_rows.get(), *ch, n * sizeof(gpsiq_chan_t), hipMemcpyDeviceToHost));
    *ch = c->h_rows.get();
    return GPSIQ_OK;
}

static int generate_batch(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, SrcKind kind, int nblocks, int nchan, int nsamp,
                          double fs, int sample_size, void *dst, int dst_is_device, double *carr_phase_out)
{
    int rc = GPSIQ_OK;
    {   // descriptors quantised / evaluated on the device (gpsiq_evaldev.cpp) where that path takes the call
        int handled = 0;
        rc = gpsiq_generate_device(c, ch, kind, nblocks, nchan, nsamp, fs, sample_size, dst, dst_is_device, carr_phase_out, nullptr, &handled);
        if (handled) return rc;
    }
    // from here on the host reads ch
    if (kind == kSrcDevice && (rc = rows_to_host(c, &ch, (size_t) nblocks * (size_t) nchan)) != GPSIQ_OK) return rc;
    if (c->nco_mode == GPSIQ_NCO_REFERENCE)
        return gpsiq_generate_reference_host(c, ch, nblocks, nchan, nsamp, fs, sample_size, dst, dst_is_device, carr_phase_out);
    const char *trace_env = std::getenv("GPSIQ_TRACE");
    const bool trace = trace_env != nullptr, trace_pieces = trace && std::atoi(trace_env) >= 2;
    const double t0 = trace ? gpsiq_wall_ms() : 0.0;
    // continue a previous call exactly where the caller hands back what it was given
    bool cont0[GPSIQ_MAX_CHAN];
    for (int i = 0; i < nchan; ++i) cont0[i] = gpsiq_continues(c, i, ch[i]);
    uint64_t carry[GPSIQ_MAX_CHAN] = {};
    int prev_prn[GPSIQ_MAX_CHAN] = {};
    const size_t blk_bytes = block_bytes(nsamp, sample_size);
    const int piece = batch_piece_blocks(nblocks, nsamp, piece_blocks_env());
    if (dst_is_device && !(blk_bytes & 15) && !((uintptr_t) dst & 3) && piece < nblocks && nsamp > 0) {
        // A long batch into device memory: quantise (= range-check), compact and upload piece k+1 on host threads under the
        // kernel of piece k; small pieces at both ends (piece_ends: nothing renders before the first piece is through, and the
        // last kernel is all that is left when the host is).  The carrier prefix goes from piece to piece exactly as it goes
        // from call to call.  A descriptor that fails its range check in a LATE piece fails the call after earlier pieces have
        // been rendered: dst and the resident set are then undefined, the carried phases untouched (include/gpsiq.h says so;
        // checking the whole timeline before the first launch was measured at 15 % of the call, 314 -> 265 G samples/s).
        bool cont[GPSIQ_MAX_CHAN];
        uint64_t seed[GPSIQ_MAX_CHAN];
        for (int i = 0; i < nchan; ++i) { cont[i] = cont0[i]; seed[i] = c->carry.phase[i]; }
        PieceOut out;                                                  // (direct: the rows are the caller's)
        rc = out.begin(c, nblocks, nsamp, sample_size, dst, dst_is_device);
        std::vector<int> ends;
        // the quantiser is a fraction of the kernel's time (kernel-bound), but nothing renders before the first piece is through
        // it: the first piece is a sixteenth of the nominal one (64 blocks at 2.6 Msps: on the device 0.1 ms into the call), each
        // later one 2.2 x the one before (GPSIQ_TRACE=2 prints the timeline)
        piece_ends(0, nblocks, piece / 8 > 0 ? piece / 8 : 1, &ends, true);
        int longest = 0;
        for (size_t k = 0; k < ends.size(); ++k) { const int nb = ends[k] - (k ? ends[k - 1] : 0); if (nb > longest) longest = nb; }
        // one piece's worth, the context's own (the set is staged out of it at once; a fresh 7 MB vector per call was 0.25 ms of
        // zero-filling before the first descriptor was looked at); every element is written by the quantiser
        std::vector<gpsiq_qchan_t> &q = c->ref_q;
        if (q.size() < (size_t) longest * (size_t) nchan) q.resize((size_t) longest * (size_t) nchan);
        for (size_t k = 0; k < ends.size() && rc == GPSIQ_OK; ++k) {
            const int b0 = k ? ends[k - 1] : 0, nb = ends[k] - b0;
            const double tq0 = trace_pieces ? gpsiq_wall_ms() : 0.0;
            rc = quantize_timeline(ch + (size_t) b0 * nchan, nb, nchan, 1.0 / fs, nsamp, cont, seed, q.data(), carry, prev_prn);
            const double tq1 = trace_pieces ? gpsiq_wall_ms() : 0.0;
            if (rc == GPSIQ_OK) rc = gpsiq_stage_descriptors(c, q.data(), nb, nchan, nullptr, 0, true);
            const double tq2 = trace_pieces ? gpsiq_wall_ms() : 0.0;
            if (rc == GPSIQ_OK) rc = gpsiq_launch_abs(c, 0, nb, nsamp, sample_size, out.target(b0), out.stride, gpsiq_piece_stream(c, (int) k), kAuto, c->call_block + (uint64_t) b0);
            if (trace_pieces)
                std::fprintf(stderr, "[gpsiq trace]   piece %zu, blocks [%d, %d): quantise from %.3f to %.3f ms, descriptors queued at %.3f, launched at %.3f\n",
                             k, b0, b0 + nb, tq0 - t0, tq1 - t0, tq2 - t0, gpsiq_wall_ms() - t0);
            for (int i = 0; i < nchan; ++i) {
                // the next piece continues a slot while it keeps its PRN and re-seeds it otherwise, as inside one timeline
                const gpsiq_chan_t *next = b0 + nb < nblocks ? &ch[(size_t) (b0 + nb) * nchan + i] : nullptr;
                cont[i] = next && next->prn > 0 && prev_prn[i] == next->prn;
                seed[i] = carry[i];
            }
        }
        rc = out.finish("batch pieces", rc);                          // on every path: the kernels write the caller's buffer
        if (rc != GPSIQ_OK) return rc;
        if (trace) std::fprintf(stderr, "[gpsiq trace] batch %d blocks in pieces of %d: whole call %.2f ms\n", nblocks, piece, gpsiq_wall_ms() - t0);
    } else {
        std::vector<gpsiq_qchan_t> &q = c->ref_q;
        if (q.size() < (size_t) nblocks * (size_t) nchan) q.resize((size_t) nblocks * (size_t) nchan);
        int qrc = quantize_timeline(ch, nblocks, nchan, 1.0 / fs, nsamp, cont0, c->carry.phase, q.data(), carry, prev_prn);
        if (qrc) return qrc;
        const double t2 = trace ? gpsiq_wall_ms() : 0.0;
        rc = gpsiq_run_to_host_or_device(c, q.data(), nblocks, nchan, nsamp, sample_size, dst, dst_is_device, c->call_block);
        if (rc) return rc;
        if (trace)
            std::fprintf(stderr, "[gpsiq trace] batch %d blocks: quantise + carrier prefix %.2f ms, upload+kernel%s %.2f ms\n",
                         nblocks, t2 - t0, dst_is_device ? "" : "+D2H", gpsiq_wall_ms() - t2);
    }
    for (int i = 0; i < nchan; ++i) gpsiq_hand_back(c, i, prev_prn[i], carry[i], carr_phase_out);      // (carry is 0 where prev_prn is: chain_carrier)
    return GPSIQ_OK;
}

// A drop-in call renders its block b as absolute block next_block + b (receiver noise) on whichever path it takes, and moves
// next_block on by nblocks when it succeeds.
int gpsiq_generate_batch(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp,
                         double fs, int sample_size, void *dst, int dst_is_device, double *carr_phase_out)
{
    int rc = gpsiq_check_gen_args(c, ch, dst, nblocks, nchan, nsamp, fs, sample_size);
    if (rc) return rc;
    if (nblocks == 0) return GPSIQ_OK;                    // an empty batch leaves the carried phases alone
    SrcKind kind;
    rc = gpsiq_rows_kind(c, ch, nullptr, &kind);          // once per call; a pointer nobody here can read: refused with nothing queued
    if (rc) return rc;
    c->call_block = c->noise.next_block;
    rc = generate_batch(c, ch, kind, nblocks, nchan, nsamp, fs, sample_size, dst, dst_is_device, carr_phase_out);
    if (rc == GPSIQ_OK) c->noise.next_block += (uint64_t) nblocks;
    return rc;
}

int gpsiq_generate_seeded(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                          const double *carr_start, void *dst, int dst_is_device)
{
    int rc = gpsiq_check_gen_args(c, ch, dst, nblocks, nchan, nsamp, fs, sample_size);
    if (rc) return rc;
    if (!carr_start && nblocks) return fail(GPSIQ_E_ARG, "null start states");
    if (nblocks == 0) return GPSIQ_OK;
    SrcKind kind;                                         // ch is host memory, pageable or page-locked: the start states are checked against it here
    rc = gpsiq_rows_kind(c, ch, "gpsiq_generate_seeded", &kind);
    if (rc) return rc;
    for (size_t k = 0; k < (size_t) nblocks * (size_t) nchan; ++k)
        if (ch[k].prn > 0 && !(carr_start[k] >= 0.0 && carr_start[k] <= 1.0)) return fail(GPSIQ_E_RANGE, "start phase %zu outside [0, 1]", k);
    c->call_block = c->noise.next_block;
    int handled = 0;
    rc = gpsiq_generate_device(c, ch, kind, nblocks, nchan, nsamp, fs, sample_size, dst, dst_is_device, nullptr, carr_start, &handled);
    if (!handled) rc = gpsiq_generate_reference_host(c, ch, nblocks, nchan, nsamp, fs, sample_size, dst, dst_is_device, nullptr, carr_start);
    if (rc == GPSIQ_OK) c->noise.next_block += (uint64_t) nblocks;
    return rc;
}
