// gpsiq_agc.cpp -- host side of gpsiq_agc and gpsiq_generate_batch_agc (include/gpsiq_rows.h, "AGC"): checks, plan (gpsiq_agc_plan.h,
// pure and answered on the CPU by tests/agc_plan.cpp), kernel look-up (gpsiq_agc_kernels.hip holds the kernels and the table of those
// that exist), the three launches, the way back of counts, multipliers and state, and the batch call's pieces.  libgpsiq_rows.so
// exports the typed calls and reaches these through the plumbing entries "agc" and "generate_batch_agc".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_agc.h"
#include "gpsiq_agc_plan.h"

using namespace gpsiq;

namespace {

int check_cfg(const gpsiq_agc_cfg_t *cfg, int sample_size, int out_sample_size)
{
    if (!cfg) return fail(GPSIQ_E_ARG, "null configuration");
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    if (cfg->window < kAgcMinWindow || cfg->window > kAgcMaxWindow || cfg->window % 64) return fail(GPSIQ_E_ARG, "window %d: a multiple of 64 in %d..%d", (int) cfg->window, kAgcMinWindow, kAgcMaxWindow);
    if (cfg->navg < 1 || cfg->navg > kAgcMaxAvg) return fail(GPSIQ_E_ARG, "navg %d outside 1..%d", (int) cfg->navg, kAgcMaxAvg);
    if (cfg->target_q8 < 1 || cfg->target_q8 > kAgcMaxTarget) return fail(GPSIQ_E_ARG, "target_q8 %u outside 1..2^23-1", (unsigned) cfg->target_q8);
    if (cfg->mult_min < 1 || cfg->mult_min > cfg->mult_max || cfg->mult_max > kAgcMaxMult || cfg->mult0 < cfg->mult_min || cfg->mult0 > cfg->mult_max)
        return fail(GPSIQ_E_ARG, "multipliers: 1 <= mult_min %u <= mult0 %u <= mult_max %u < 2^24", (unsigned) cfg->mult_min, (unsigned) cfg->mult0, (unsigned) cfg->mult_max);
    if (cfg->blank_thresh < 0 || cfg->blank_thresh > kAgcMaxThresh) return fail(GPSIQ_E_ARG, "blank_thresh %d outside 0..%d", (int) cfg->blank_thresh, kAgcMaxThresh);
    if (cfg->blank_hold < 0 || cfg->blank_hold > kAgcMaxHold) return fail(GPSIQ_E_ARG, "blank_hold %d outside 0..%d", (int) cfg->blank_hold, kAgcMaxHold);
    const int most = out_sample_size == GPSIQ_SC08 ? 127 : 32767;
    if (cfg->qmax < 1 || cfg->qmax > most) return fail(GPSIQ_E_ARG, "qmax %d outside 1..%d for %d-byte outputs", (int) cfg->qmax, most, out_sample_size);
    return GPSIQ_OK;
}

// a state that cannot have come from a call with this window and navg
int check_state(const gpsiq_agc_cfg_t *cfg, const gpsiq_agc_state_t *st)
{
    if (!st) return GPSIQ_OK;
    if (st->nring > (uint32_t) cfg->navg) return fail(GPSIQ_E_ARG, "state: nring %u above navg %d", (unsigned) st->nring, (int) cfg->navg);
    if (st->fill >= (uint32_t) cfg->window) return fail(GPSIQ_E_ARG, "state: fill %u not below the window %d", (unsigned) st->fill, (int) cfg->window);
    if (st->pcnt > 2 * st->fill) return fail(GPSIQ_E_ARG, "state: pcnt %u above 2 * fill %u", (unsigned) st->pcnt, (unsigned) st->fill);
    if (st->hold > (uint32_t) cfg->blank_hold) return fail(GPSIQ_E_ARG, "state: hold %u above blank_hold %d", (unsigned) st->hold, (int) cfg->blank_hold);
    if (st->psum > ((uint64_t) st->pcnt << 30)) return fail(GPSIQ_E_ARG, "state: psum above what pcnt %u elements can hold", (unsigned) st->pcnt);
    for (uint32_t r = 0; r < (uint32_t) kAgcMaxAvg; ++r) {
        if (r >= st->nring && (st->wsum[r] || st->wcnt[r])) return fail(GPSIQ_E_ARG, "state: ring entry %u beyond nring %u is not zero", (unsigned) r, (unsigned) st->nring);
        if (st->wcnt[r] > 2 * (uint32_t) cfg->window || st->wsum[r] > ((uint64_t) st->wcnt[r] << 30))
            return fail(GPSIQ_E_ARG, "state: ring entry %u holds more than a window of %d can", (unsigned) r, (int) cfg->window);
    }
    return GPSIQ_OK;
}

void note_plan(gpsiq_ctx *c, const AgcPlan &p, long long pieces)
{
    long long *o = c->agc.last;
    o[0] = p.launch ? (long long) p.measure_grid : -1; o[1] = kAgcTile; o[2] = (long long) p.gains_grid; o[3] = (long long) p.apply_grid;
    o[4] = kAgcApplyTile; o[5] = pieces;
}

// counts zeroed and the state a call starts from in st[0], queued on s.  The caller has made sure nothing queued earlier still reads
// h_back (every call ends synchronised)
int stage_state(gpsiq_ctx *c, const gpsiq_agc_state_t *state, hipStream_t s)
{
    AgcSet &k = c->agc;
    std::memset(k.h_back.get(), 0, sizeof(AgcBack));
    if (state) k.h_back[0].st[0] = *state;
    HIP_TRY(hipMemcpyAsync(k.d_back.get(), k.h_back.get(), sizeof(AgcBack), hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

// the three launches of a span queued on s: st[from] in, st[from ^ 1] out.  The counts are NOT zeroed here (the batch call adds its
// pieces up); the slots are, per launch.  timed: the set's events are recorded in front of the first launch and behind each
int queue_agc(gpsiq_ctx *c, const AgcPlan &p, int nsamp, int sample_size, const uint8_t *src, const gpsiq_agc_cfg_t &cfg, uint32_t fill, int from,
              int out_sample_size, uint8_t *dst, hipStream_t s, bool timed)
{
    AgcSet &k = c->agc;
    const AgcMeasureFn measure = agc_measure_kernel(sample_size, p.mask);
    const AgcGainsFn gains = agc_gains_kernel();
    const AgcApplyFn apply = agc_apply_kernel(sample_size, out_sample_size, p.mask);
    if (!measure || !gains || !apply) return fail(GPSIQ_E_DEVICE, "no gain control kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
    uint8_t *scratch = k.d_scratch.get();
    unsigned long long *wsum = reinterpret_cast<unsigned long long *>(scratch);
    uint32_t *wcnt = reinterpret_cast<uint32_t *>(scratch + p.off_cnt), *mults = reinterpret_cast<uint32_t *>(scratch + p.off_mult);
    uint8_t *mask = p.mask ? scratch + p.off_mask : nullptr;
    AgcBack *back = k.d_back.get();
    const gpsiq_agc_state_t *st_in = &back->st[from];
    gpsiq_agc_state_t *st_out = &back->st[from ^ 1];
    const AgcGain g = {cfg.target_q8, cfg.mult0, cfg.mult_min, cfg.mult_max, cfg.navg};
    HIP_TRY(hipMemsetAsync(scratch, 0, p.zero_bytes, s));
    if (timed) HIP_TRY(hipEventRecord(k.t[0].get(), s));
    hipLaunchKernelGGL(measure, dim3(p.measure_grid), dim3(p.threads), 0, s, src, nsamp, fill, (uint32_t) cfg.window, (int) cfg.blank_thresh, (int) cfg.blank_hold,
                       st_in, st_out, wsum, wcnt, mask, &back->blanked);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(k.t[1].get(), s));
    hipLaunchKernelGGL(gains, dim3(p.gains_grid), dim3(p.threads), 0, s, (uint32_t) p.nwin, nsamp, fill, (uint32_t) cfg.window, g, p.mask ? 1 : 0, st_in, st_out,
                       (const unsigned long long *) wsum, (const uint32_t *) wcnt, mults);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(k.t[2].get(), s));
    hipLaunchKernelGGL(apply, dim3(p.apply_grid), dim3(p.threads), 0, s, src, nsamp, fill, (uint32_t) cfg.window, (const uint32_t *) mults, (const uint8_t *) mask,
                       st_in, (int) cfg.qmax, dst, p.units, &back->clipped);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(k.t[3].get(), s));
    return GPSIQ_OK;
}

}  // namespace

int gpsiq_agc_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, const gpsiq_agc_cfg_t *cfg, gpsiq_agc_state_t *state, int out_sample_size,
                   void *dst, void *hip_stream, uint32_t *mults, uint64_t *clipped, uint64_t *blanked, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_cfg(cfg, sample_size, out_sample_size)) return rc;
    if (int rc = check_state(cfg, state)) return rc;
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if ((!src || !dst) && nsamp) return fail(GPSIQ_E_ARG, "null %s", src ? "destination" : "source");
    if ((uintptr_t) src & 3) return fail(GPSIQ_E_ARG, "source %p not 4-byte aligned", src);
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    const size_t src_len = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, dst_len = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    if (overlap(dst, dst_len, src, src_len)) return fail(GPSIQ_E_ARG, "source [%p, +%zu) and destination [%p, +%zu) overlap", src, src_len, dst, dst_len);
    const uint32_t fill = state ? state->fill : 0;
    const AgcPlan p = plan_agc(nsamp, cfg->window, fill, cfg->blank_thresh > 0);
    if (clipped) *clipped = 0;
    if (blanked) *blanked = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    note_plan(c, p, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: counts of 0, the state as it was
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    AgcSet &k = c->agc;
    if (int rc = k.reserve(p.scratch_bytes)) return rc;
    if (int rc = stage_state(c, state, s)) return rc;
    if (int rc = queue_agc(c, p, nsamp, sample_size, static_cast<const uint8_t *>(src), *cfg, fill, 0, out_sample_size, static_cast<uint8_t *>(dst), s, true)) return rc;
    HIP_TRY(hipMemcpyAsync(k.h_back.get(), k.d_back.get(), sizeof(AgcBack), hipMemcpyDeviceToHost, s));
    if (mults) HIP_TRY(hipMemcpyAsync(mults, k.d_scratch.get() + p.off_mult, sizeof(uint32_t) * (size_t) p.nwin, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (clipped) *clipped = (uint64_t) k.h_back[0].clipped;
    if (blanked) *blanked = (uint64_t) k.h_back[0].blanked;
    if (state) *state = k.h_back[0].st[1];
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&k.last_ms[i], k.t[i].get(), k.t[i + 1].get()));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, k.t[0].get(), k.t[3].get()));
    return GPSIQ_OK;
}

// The pieces of gpsiq_stage_batch.h with this stage in the filter's place: no lead region, no history -- what a piece needs of the
// stream before it is the state, which stays on the device: piece p reads st[p & 1] and leaves st[(p + 1) & 1], and the block with both
// counts and both states comes back once, as the loop's counter, behind the last piece.  The fill before a piece is host arithmetic.
// Every piece is a whole number of blocks, so a piece's outputs are its blocks' rows back to back.
int gpsiq_generate_batch_agc_impl(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                                  const gpsiq_agc_cfg_t *cfg, gpsiq_agc_state_t *state, int out_sample_size, void *dst, size_t dst_block_stride,
                                  uint64_t *clipped, uint64_t *blanked, double *carr_phase_out)
{
    if (!c || (!ch && nblocks) || (!dst && nblocks && nsamp)) return fail(GPSIQ_E_ARG, "null argument");
    if (int rc = check_cfg(cfg, sample_size, out_sample_size)) return rc;
    if (int rc = check_state(cfg, state)) return rc;
    if (int rc = check_batch_shape(nblocks, nchan, nsamp, fs)) return rc;
    const size_t blk_bytes = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, row_bytes = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    if (dst_block_stride < row_bytes) return fail(GPSIQ_E_ARG, "block stride %zu too small", dst_block_stride);
    if (clipped) *clipped = 0;
    if (blanked) *blanked = 0;
    if (nblocks == 0) return GPSIQ_OK;                                // an empty batch leaves the carried phases and the state alone
    const char *env = std::getenv("GPSIQ_AGC_PIECE_BLOCKS");
    const int piece = agc_piece_blocks(nblocks, nsamp, blk_bytes, env ? std::atol(env) : 0);
    const bool mask = cfg->blank_thresh > 0;
    const uint32_t fill0 = state ? state->fill : 0;
    // the largest scratch a piece asks for: a full piece at the fill that touches the most windows
    const AgcPlan whole = plan_agc(piece * nsamp, cfg->window, (uint32_t) cfg->window - 1, mask);
    if (int rc = gpsiq_stage_batch_begin(c, "gpsiq_generate_batch_agc", ch, blk_bytes * (size_t) piece + 4, row_bytes * (size_t) piece + 4)) return rc;     // (+4: never a request of no bytes)
    AgcSet &k = c->agc;
    if (int rc = k.reserve(whole.scratch_bytes)) return rc;
    StageBatch stage = {"gain-controlled batch", sample_size, 0, 0, piece, &k.d_back.get()->clipped, &k.h_back.get()->clipped};
    stage.count_words = sizeof(AgcBack) / sizeof(unsigned long long);
    const int npieces = (nblocks + piece - 1) / piece;
    note_plan(c, plan_agc(piece * nsamp, cfg->window, fill0, mask), npieces);
    const hipStream_t ss = c->ring.stage_stream.get();
    const int rc0 = !nsamp ? GPSIQ_OK : stage_state(c, state, ss);
    double carr[GPSIQ_MAX_CHAN] = {};
    uint64_t clamped = 0;
    const int rc = gpsiq_stage_batch_run(c, stage, rc0, ch, nblocks, nchan, nsamp, fs, [&](const Piece &pc, PieceCopy *cp) -> int {
        uint8_t *out = c->ring.d_out[pc.pair].get();
        const uint32_t fill = (uint32_t) (((uint64_t) fill0 + (uint64_t) pc.b0 * (uint64_t) nsamp) % (uint64_t) cfg->window);
        const AgcPlan pl = plan_agc(pc.nb * nsamp, cfg->window, fill, mask);
        if (int rq = queue_agc(c, pl, pc.nb * nsamp, sample_size, pc.span, *cfg, fill, pc.p & 1, out_sample_size, out, ss, false)) return rq;
        *cp = {out, row_bytes, row_bytes, (size_t) pc.nb, static_cast<uint8_t *>(dst) + (size_t) pc.b0 * dst_block_stride, dst_block_stride};
        return GPSIQ_OK;
    }, carr, &clamped);
    if (rc != GPSIQ_OK) return rc;
    if (clipped) *clipped = clamped;
    if (nsamp) {
        if (blanked) *blanked = (uint64_t) k.h_back[0].blanked;
        if (state) *state = k.h_back[0].st[npieces & 1];
    }
    if (carr_phase_out) std::memcpy(carr_phase_out, carr, sizeof(double) * (size_t) nchan);
    return GPSIQ_OK;
}

extern "C" int gpsiq_agc_last_plan(const gpsiq_ctx_t *c, long long out[6])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 6; ++i) out[i] = c->agc.last[i];
    return GPSIQ_OK;
}

extern "C" int gpsiq_agc_last_ms(const gpsiq_ctx_t *c, float out[3])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 3; ++i) out[i] = c->agc.last_ms[i];
    return GPSIQ_OK;
}
