// gpsiq_multi.cpp -- gpsiq_generate_batch_multi (include/gpsiq.h): one timeline over several contexts, one contiguous block range
// each, rendered concurrently.  The host side of the timeline (quantiser / reference walk) runs once; every non-empty range has a
// host thread that renders it on its context's device.  HIP runtime only.
#include <hip/hip_runtime.h>

#include <vector>

#include "gpsiq_calls.h"
#include "gpsiq_ctx.h"

using namespace gpsiq;

namespace {

// what every range of one call shares
struct Call { const gpsiq_qchan_t *q; int nchan, nsamp, ss; };

// a piece of the reference walk on its way to the range that owns it: blocks [b0, b0 + nb) of the range
struct Piece { const gpsiq_qchan_t *q = nullptr; int b0 = 0, nb = 0; std::vector<gpsiq_patch_t> patches; };

// One row of the call's table: the context, its blocks [first, first + nb) of the timeline, where they go, and the absolute index
// of the range's first block (ctx[0]'s numbering, for the receiver noise) -- and the body that renders the range, on a thread of
// its own where one can be started.
struct Range {
    gpsiq_ctx *c = nullptr;
    int        first = 0, nb = 0, dst_is_device = 0;
    void      *dst = nullptr;
    uint64_t   nbase = 0;
    const Call *call = nullptr;
    Status     st;                                      // the body's outcome; the thread that feeds the walk polls it
    WorkQueue<Piece> pieces;                            // GPSIQ_NCO_REFERENCE: what the walk hands this range

    void run(void (*fn)(Range &), bool own_thread)
    {
        body = fn;
        started = own_thread && pthread_create(&th, nullptr, [](void *p) -> void * { Range &r = *static_cast<Range *>(p); r.body(r); return nullptr; }, this) == 0;
    }
    void join()
    {
        if (started) pthread_join(th, nullptr);
        else if (body) body(*this);                     // no thread of its own, or none could be started: do it here
        body = nullptr;
    }
private:
    void (*body)(Range &) = nullptr;
    pthread_t th; bool started = false;
};

// every body has returned; the first range that failed is the call's error
int join_all(std::vector<Range> &ranges)
{
    for (Range &r : ranges) r.join();
    for (size_t i = 0; i < ranges.size(); ++i)
        if (!ranges[i].st.ok()) return fail(ranges[i].st.code(), "device range %d: %s", (int) i, ranges[i].st.text);
    return GPSIQ_OK;
}

void render_fixed_range(Range &r)
{
    r.st.take(gpsiq_run_to_host_or_device(r.c, r.call->q + (size_t) r.first * r.call->nchan, r.nb, r.call->nchan, r.call->nsamp, r.call->ss, r.dst,
                                          r.dst_is_device, r.nbase));
}

void render_reference_range(Range &r)
{
    PieceOut out;
    r.st.take(out.begin(r.c, r.nb, r.call->nsamp, r.call->ss, r.dst, r.dst_is_device));
    Piece it;
    for (int k = 0; r.pieces.pop(&it); ++k)
        if (r.st.ok())                                  // after an error: take the rest off the queue, render nothing
            r.st.take(gpsiq_ref_piece(r.c, out, k, it.q, it.b0, it.nb, r.call->nchan, r.call->nsamp, r.call->ss, r.nbase, it.patches));
    r.st.take(out.finish("reference NCO pieces"));
}

// the fixed-point model: the host side once, for the whole timeline (threaded), then every device its range -- one host thread per
// context, the first range on this one
int render_fixed(std::vector<Range> &ranges, const gpsiq_chan_t *ch, int nblocks, double fs, std::vector<gpsiq_qchan_t> &q, double *carr_phase_out)
{
    gpsiq_ctx *c0 = ranges[0].c;
    const Call &call = *ranges[0].call;
    uint64_t carry[GPSIQ_MAX_CHAN] = {};
    int prev_prn[GPSIQ_MAX_CHAN] = {};
    bool cont0[GPSIQ_MAX_CHAN];
    for (int i = 0; i < call.nchan; ++i) cont0[i] = gpsiq_continues(c0, i, ch[i]);
    int rc = quantize_timeline(ch, nblocks, call.nchan, 1.0 / fs, call.nsamp, cont0, c0->carry.phase, q.data(), carry, prev_prn);
    if (rc) return rc;
    for (size_t i = 0; i < ranges.size(); ++i)
        if (ranges[i].nb > 0) ranges[i].run(render_fixed_range, i > 0);
    rc = join_all(ranges);
    if (rc) return rc;
    for (int i = 0; i < call.nchan; ++i) gpsiq_hand_back(c0, i, prev_prn[i], carry[i], carr_phase_out);      // (carry is 0 where prev_prn is: chain_carrier)
    return GPSIQ_OK;
}

// GPSIQ_NCO_REFERENCE.  The walk is serial in time, the devices are not: the walkers (one host thread per channel, RefWalk) go
// through the whole timeline once, and this thread hands every piece, as soon as all channels are through it, to the device that
// owns it; device i starts as soon as the walk reaches its range, and renders under the walk of what follows.
int render_reference(std::vector<Range> &ranges, const gpsiq_chan_t *ch, int nblocks, double fs, std::vector<gpsiq_qchan_t> &q, double *carr_phase_out)
{
    gpsiq_ctx *c0 = ranges[0].c;
    const Call &call = *ranges[0].call;
    const int nchan = call.nchan, nsamp = call.nsamp;
    // pieces never straddle two devices' ranges
    std::vector<int> ends, owner;
    for (int i = 0; i < (int) ranges.size(); ++i) {
        Range &r = ranges[(size_t) i];
        if (r.nb == 0) continue;
        r.run(render_reference_range, true);
        const size_t before = ends.size();
        piece_ends(r.first, r.nb, ref_chunk_blocks(r.nb, nsamp, piece_blocks_env()), &ends, ref_kernel_bound(nsamp, nchan, gpsiq_rate_kernel(), host_threads()));
        owner.insert(owner.end(), ends.size() - before, i);
    }
    // the carrier chain: level 1 of the whole timeline on the first device (one launch; a GPU walks an hour of config 5 in
    // milliseconds where sixteen host threads took a tenth of a second), the link inside the walkers' chain tasks
    const bool dev_chain = gpsiq_chain_on_device(nblocks, nsamp, nchan);
    int crc = GPSIQ_OK;
    if (dev_chain) {
        crc = hipSetDevice(c0->device) == hipSuccess ? c0->chain.reserve((size_t) nblocks * (size_t) nchan) : fail(GPSIQ_E_DEVICE, "hipSetDevice");
        if (crc == GPSIQ_OK) {
            gpsiq_chain_stage_inputs(c0, ch, 0, nblocks, nchan);
            crc = gpsiq_chain_maps_staged(c0, nblocks, nchan, fs, nsamp, nullptr, 0, nullptr);
        }
    }
    RefWalk w(ch, nblocks, nchan, 1.0 / fs, nsamp, q.data(), nullptr, nullptr, ends);
    if (dev_chain && crc == GPSIQ_OK) { w.in = c0->chain.h_in.get(); w.maps = c0->chain.h_maps.get(); }     // (a failed level 1: the serial walk)
    Status walked;
    {
        WalkThread walk(w);
        int open = 0;                                           // ranges before this one have all their pieces
        for (size_t k = 0; k < w.npieces(); ++k) {
            if (walked.ok()) {
                walked.take(w.wait_piece(k), w.err);
                for (Range &r : ranges)                         // a device that has failed: stop walking for it
                    if (!r.st.ok()) w.abort();
            }
            for (; open < owner[k]; ++open) ranges[(size_t) open].pieces.close();     // the walk has left this range: no more pieces for it
            if (!walked.ok()) continue;
            Range &r = ranges[(size_t) owner[k]];
            Piece it;
            const int b0 = k ? w.ends[k - 1] : 0;
            it.nb = w.ends[k] - b0;
            it.b0 = b0 - r.first;
            it.q = q.data() + (size_t) b0 * nchan;
            w.take_patches(k, &it.patches, true);
            r.pieces.push(std::move(it));
        }
        for (; open < (int) ranges.size(); ++open) ranges[(size_t) open].pieces.close();
    }
    const int rc = join_all(ranges);
    if (!walked.ok()) return walked.fail();
    if (rc) return rc;
    if (carr_phase_out)
        for (int i = 0; i < nchan; ++i) carr_phase_out[i] = w.last_prn[i] ? w.carr_end[i] : ch[(size_t) (nblocks - 1) * nchan + i].carr_phase;
    return GPSIQ_OK;
}

// Every range is rendered with ctx[0]'s noise and level settings and numbering (device i from next_block + begin_i): the other
// contexts take ctx[0]'s seed, sigma and level for the call and get their own back after it, whatever became of the call.
struct BorrowedSettings {
    BorrowedSettings(gpsiq_ctx_t *const *ctx_, int ndev_) : ctx(ctx_), ndev(ndev_), noise((size_t) ndev_), level((size_t) ndev_)
    {
        for (int i = 0; i < ndev; ++i) { noise[(size_t) i] = ctx[i]->noise; level[(size_t) i] = ctx[i]->level; }
    }
    int lend()
    {
        const gpsiq_ctx::Noise &n0 = ctx[0]->noise;
        int rc = GPSIQ_OK;
        for (int i = 1; i < ndev && rc == GPSIQ_OK; ++i) {
            if (ctx[i]->noise.seed != n0.seed || ctx[i]->noise.sigma != n0.sigma) rc = gpsiq_apply_noise(ctx[i], n0.seed, n0.sigma);
            if (rc == GPSIQ_OK) rc = gpsiq_apply_level(ctx[i], ctx[0]->level.mult, ctx[0]->level.qmax);
        }
        return rc;
    }
    int restore(int rc)     // rc: what became of the call, whose error text stands; a failed restore of a good call is reported
    {
        Status call;
        call.take(rc);
        for (int i = 1; i < ndev; ++i) {
            ctx[i]->level = level[(size_t) i];
            const gpsiq_ctx::Noise &o = noise[(size_t) i];
            if (ctx[i]->noise.seed != o.seed || ctx[i]->noise.sigma != o.sigma) call.take(gpsiq_apply_noise(ctx[i], o.seed, o.sigma));
        }
        return call.ok() ? GPSIQ_OK : call.fail();
    }
private:
    gpsiq_ctx_t *const *ctx; int ndev;
    std::vector<gpsiq_ctx::Noise> noise;                // every context's own, as the call found them
    std::vector<gpsiq_ctx::Level> level;
};

}  // namespace

int gpsiq_generate_batch_multi(gpsiq_ctx_t *const *ctx, int ndev, const gpsiq_chan_t *ch, int nblocks, int nchan,
                               int nsamp, double fs, int sample_size, void *host_dst, void *const *dev_dst,
                               double *carr_phase_out)
{
    if (!ctx || ndev < 1 || ndev > 64) return fail(GPSIQ_E_ARG, "bad device list");
    for (int i = 0; i < ndev; ++i) {
        if (!ctx[i]) return fail(GPSIQ_E_ARG, "null context %d", i);
        for (int j = 0; j < i; ++j)
            if (ctx[j] == ctx[i]) return fail(GPSIQ_E_ARG, "context %d listed twice: the ranges are rendered concurrently, one context each", i);
    }
    if (!host_dst && !dev_dst) return fail(GPSIQ_E_ARG, "no destination");
    int rc = gpsiq_check_gen_args(ctx[0], ch, host_dst ? host_dst : (void *) dev_dst, nblocks, nchan, nsamp, fs, sample_size);
    if (rc) return rc;
    if (nblocks == 0) return GPSIQ_OK;
    rc = gpsiq_rows_kind(ctx[0], ch, "gpsiq_generate_batch_multi", nullptr);     // the host side of the timeline runs once, here: ch is host memory
    if (rc) return rc;
    // the ranges, once: everything after reads this table
    std::vector<gpsiq_qchan_t> q((size_t) nblocks * (size_t) nchan);
    const Call call = {q.data(), nchan, nsamp, sample_size};
    std::vector<Range> ranges((size_t) ndev);
    for (int i = 0; i < ndev; ++i) {
        Range &r = ranges[(size_t) i];
        int b1 = 0;
        (void) gpsiq_shard_range(nblocks, i, ndev, &r.first, &b1);
        r.c = ctx[i]; r.nb = b1 - r.first; r.call = &call;
        r.dst = host_dst ? (void *) (static_cast<uint8_t *>(host_dst) + (size_t) r.first * block_bytes(nsamp, sample_size)) : dev_dst[i];
        r.dst_is_device = host_dst ? 0 : 1;
        r.nbase = ctx[0]->noise.next_block + (uint64_t) r.first;    // ctx[0]'s numbering (and noise settings) for every range
        if (r.nb > 0 && !r.dst) return fail(GPSIQ_E_ARG, "null destination for range %d", i);
    }
    BorrowedSettings own(ctx, ndev);
    rc = own.lend();
    if (rc == GPSIQ_OK)
        rc = ctx[0]->nco_mode == GPSIQ_NCO_REFERENCE ? render_reference(ranges, ch, nblocks, fs, q, carr_phase_out)
                                                     : render_fixed(ranges, ch, nblocks, fs, q, carr_phase_out);
    if (rc == GPSIQ_OK) ctx[0]->noise.next_block += (uint64_t) nblocks;
    return own.restore(rc);
}
