// gpsiq_resample.cpp -- host side of gpsiq_resample and gpsiq_generate_batch_resampled (include/gpsiq_rows.h, "Resample"): checks,
// plan (gpsiq_resample_plan.h, pure and pinned on the CPU), the tap table on its way to the device, kernel look-up
// (gpsiq_resample_kernels.hip holds the kernels and the table of those that exist), launch, count, and the batch call's pieces.
// libgpsiq_rows.so exports the typed calls and reaches these through the plumbing entries "resample" and "generate_batch_resampled".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_resample.h"
#include "gpsiq_resample_plan.h"

using namespace gpsiq;

namespace {

// what both calls ask of the table, the step and the formats
int check_table(const int16_t *taps, int log2_phases, int ntaps, int shift, int interp, uint64_t step, uint64_t pos0, int sample_size, int out_sample_size)
{
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    if (log2_phases < 0 || log2_phases > kRsMaxLog2Phases) return fail(GPSIQ_E_ARG, "log2_phases %d outside 0..%d", log2_phases, kRsMaxLog2Phases);
    if (ntaps < 1 || ntaps > kRsMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kRsMaxTaps);
    const int rows = (1 << log2_phases) + 1;
    if (rows * ntaps > kRsMaxTable) return fail(GPSIQ_E_ARG, "%d rows of %d taps: more than %d entries", rows, ntaps, kRsMaxTable);
    if (shift < 0 || shift > kRsMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kRsMaxShift);
    if (interp != 0 && interp != 1) return fail(GPSIQ_E_ARG, "interp %d: 0 or 1", interp);
    if (step < kRsMinStep || step > kRsMaxStep) return fail(GPSIQ_E_ARG, "step %llu outside 2^29..2^35", (unsigned long long) step);
    if (pos0 >= kRsMaxPos) return fail(GPSIQ_E_ARG, "pos0 %llu: 2^63 or more", (unsigned long long) pos0);
    if (!taps) return fail(GPSIQ_E_ARG, "null taps");
    for (int r = 0; r < rows; ++r) {
        long mag = 0;
        for (int k = 0; k < ntaps; ++k) { const long t = taps[(size_t) r * (size_t) ntaps + (size_t) k]; mag += t < 0 ? -t : t; }
        if (mag > kRsTapSum) return fail(GPSIQ_E_RANGE, "row %d: sum |taps| %ld above %ld: the accumulator would not hold the sum", r, mag, kRsTapSum);
    }
    return GPSIQ_OK;
}

static_assert(kRsAuto == 0 && kRsForceGeneric == 1 && kRsForceRows == 2, "forced_kernel's values (gpsiq_stage_call.h)");

void note_plan(gpsiq_ctx *c, const ResamplePlan &p, long long pieces)
{
    c->rs.last[0] = p.launch ? (long long) p.kernel : -1; c->rs.last[1] = (long long) p.grid; c->rs.last[2] = (long long) p.run; c->rs.last[3] = pieces;
}

// The table of a call, page-locked, then queued for the device on s.  The caller has made sure nothing queued earlier still reads
// h_taps (every call ends synchronised).
int stage_table(gpsiq_ctx *c, const int16_t *taps, int log2_phases, int ntaps, hipStream_t s)
{
    ResampleSet &k = c->rs;
    const size_t entries = (size_t) ((1 << log2_phases) + 1) * (size_t) ntaps;
    std::memcpy(k.h_taps.get(), taps, entries * sizeof(int16_t));
    HIP_TRY(hipMemcpyAsync(k.d_taps.get(), k.h_taps.get(), entries * sizeof(int16_t), hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

// the resampler queued on s behind its table: the counter is NOT zeroed here (the batch call adds its pieces up)
int queue_resample(gpsiq_ctx *c, const ResamplePlan &p, int nsamp, int sample_size, const uint8_t *src, const uint8_t *head, int log2_phases, int ntaps,
                   int shift, int interp, uint64_t step, uint64_t pos0, int out_sample_size, uint8_t *dst, hipStream_t s)
{
    ResampleSet &k = c->rs;
    if (p.kernel == kRsRows) {
        const ResampleRowsFn kernel = resample_rows_kernel(sample_size, out_sample_size, p.pad);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no row resampler kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, (const int16_t *) k.d_taps.get(), log2_phases, ntaps, shift, interp,
                           step, pos0, dst, p.nout, p.run, p.runs, k.clip.d_count.get());
    } else {
        const ResampleGenericFn kernel = resample_generic_kernel(sample_size, out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no resampler kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, (const int16_t *) k.d_taps.get(), log2_phases, ntaps, shift, interp,
                           step, pos0, dst, p.nout, p.runs, k.clip.d_count.get());
    }
    HIP_TRY(hipGetLastError());
    return GPSIQ_OK;
}

}  // namespace

int gpsiq_resample_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, const void *head, const int16_t *taps, int log2_phases, int ntaps,
                        int shift, int interp, uint64_t step, uint64_t pos0, int out_sample_size, void *dst, void *hip_stream, uint64_t *nout,
                        uint64_t *next_pos, uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_table(taps, log2_phases, ntaps, shift, interp, step, pos0, sample_size, out_sample_size)) return rc;
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    const ResamplePlan p = plan_resample((uint64_t) nsamp, log2_phases, ntaps, step, pos0, forced_kernel("GPSIQ_RESAMPLE_KERNEL", "rows"));
    if (int rc = check_span(src, nsamp, sample_size, head, ntaps, dst, p.nout, out_sample_size)) return rc;
    if (nout) *nout = p.nout;
    if (next_pos) *next_pos = p.next_pos;
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    note_plan(c, p, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no output: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    ResampleSet &k = c->rs;
    if (int rc = k.reserve()) return rc;
    if (int rc = stage_table(c, taps, log2_phases, ntaps, s)) return rc;
    return counted_call(k.clip, s, [&] {
        return queue_resample(c, p, nsamp, sample_size, static_cast<const uint8_t *>(src), static_cast<const uint8_t *>(head), log2_phases, ntaps, shift,
                              interp, step, pos0, out_sample_size, static_cast<uint8_t *>(dst), s);
    }, clipped, kernel_ms);
}

// The pieces of gpsiq_stage_batch.h with the resampler as the stage: lead region and history as the filtered call's
// (gpsiq_filter.cpp), the first piece's history zeros, written per call.  The position crosses on the host: piece p + 1 starts at
// piece p's next_pos, also where piece p gave no output (nothing is launched for it); a piece's outputs are one run of samples and
// cross to where the pieces before ended.
int gpsiq_generate_batch_resampled_impl(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                                        const int16_t *taps, int log2_phases, int ntaps, int shift, int interp, uint64_t step, uint64_t pos0,
                                        int out_sample_size, void *dst, uint64_t dst_capacity, uint64_t *nout, uint64_t *clipped, double *carr_phase_out)
{
    if (!c || (!ch && nblocks)) return fail(GPSIQ_E_ARG, "null argument");
    if (int rc = check_table(taps, log2_phases, ntaps, shift, interp, step, pos0, sample_size, out_sample_size)) return rc;
    if (int rc = check_batch_shape(nblocks, nchan, nsamp, fs)) return rc;
    uint64_t total = 0, end_pos = 0;
    resample_span((uint64_t) nblocks * (uint64_t) nsamp, pos0, step, &total, &end_pos);
    if (dst_capacity < total) return fail(GPSIQ_E_ARG, "room for %llu samples, the call writes %llu", (unsigned long long) dst_capacity, (unsigned long long) total);
    if (!dst && total) return fail(GPSIQ_E_ARG, "null destination");
    if (clipped) *clipped = 0;
    if (nout) *nout = 0;
    if (nblocks == 0) return GPSIQ_OK;                                // an empty batch leaves the carried phases alone
    const size_t blk_bytes = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, out_sample_bytes = (size_t) 2 * (size_t) out_sample_size;
    const char *env = std::getenv("GPSIQ_RESAMPLE_PIECE_BLOCKS");
    const int piece = resample_piece_blocks(nblocks, nsamp, blk_bytes, env ? std::atol(env) : 0);
    const size_t hist = (size_t) 2 * (size_t) (ntaps - 1) * (size_t) sample_size, hb = (hist + 15) & ~(size_t) 15;
    const int force = forced_kernel("GPSIQ_RESAMPLE_KERNEL", "rows");
    const size_t piece_out = (size_t) resample_piece_outputs((uint64_t) piece * (uint64_t) nsamp, step) * out_sample_bytes;
    if (int rc = gpsiq_stage_batch_begin(c, "gpsiq_generate_batch_resampled", ch, hb + blk_bytes * (size_t) piece + 4, piece_out + 4)) return rc;     // (+4: never a request of no bytes)
    ResampleSet &k = c->rs;
    if (int rc = k.reserve()) return rc;
    const StageBatch stage = {"resampled batch", sample_size, hb, hist, piece, k.clip.d_count.get(), k.clip.h_count.get()};
    note_plan(c, plan_resample((uint64_t) piece * (uint64_t) nsamp, log2_phases, ntaps, step, pos0, force), (nblocks + piece - 1) / piece);
    const hipStream_t ss = c->ring.stage_stream.get();
    const int rc0 = !nsamp ? GPSIQ_OK : [&]() -> int {
        if (int rc = stage_table(c, taps, log2_phases, ntaps, ss)) return rc;
        HIP_TRY(hipMemsetAsync(k.clip.d_count.get(), 0, sizeof(unsigned long long), ss));
        if (hb) HIP_TRY(hipMemsetAsync(c->ring.d_render[0].get(), 0, hb, ss));       // the first block's history
        return GPSIQ_OK;
    }();
    double carr[GPSIQ_MAX_CHAN] = {};
    uint64_t pos = pos0, done = 0, clamped = 0;
    const int rc = gpsiq_stage_batch_run(c, stage, rc0, ch, nblocks, nchan, nsamp, fs, [&](const Piece &pc, PieceCopy *cp) -> int {
        uint8_t *out = c->ring.d_out[pc.pair].get();
        const ResamplePlan pl = plan_resample((uint64_t) pc.nb * (uint64_t) nsamp, log2_phases, ntaps, step, pos, force);
        if (pl.launch)
            if (int rq = queue_resample(c, pl, pc.nb * nsamp, sample_size, pc.span, hist ? pc.span - hist : nullptr, log2_phases, ntaps, shift, interp, step, pos,
                                        out_sample_size, out, ss)) return rq;
        const size_t bytes = (size_t) pl.nout * out_sample_bytes;
        *cp = {out, bytes, bytes, pl.nout ? (size_t) 1 : 0, static_cast<uint8_t *>(dst) + (size_t) done * out_sample_bytes, bytes};
        pos = pl.next_pos;
        done += pl.nout;
        return GPSIQ_OK;
    }, carr, &clamped);
    if (rc != GPSIQ_OK) return rc;
    if (done != total) return fail(GPSIQ_E_DEVICE, "resampled batch: the pieces gave %llu samples, the span has %llu", (unsigned long long) done, (unsigned long long) total);
    if (clipped) *clipped = clamped;
    if (nout) *nout = total;
    if (carr_phase_out) std::memcpy(carr_phase_out, carr, sizeof(double) * (size_t) nchan);
    return GPSIQ_OK;
}

extern "C" int gpsiq_resample_last_plan(const gpsiq_ctx_t *c, long long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->rs.last[i];
    return GPSIQ_OK;
}
