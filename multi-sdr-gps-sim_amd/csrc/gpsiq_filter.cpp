// gpsiq_filter.cpp -- host side of gpsiq_filter and gpsiq_generate_batch_filtered (include/gpsiq_rows.h, "Filter"): checks, plan
// (gpsiq_filter_plan.h, pure and pinned on the CPU), the taps and the matrix kernel's digit planes on their way to the device, kernel
// look-up (gpsiq_filter_kernels.hip holds the kernels and the table of those that exist), launch, count, and the batch call's pieces.
// libgpsiq_rows.so exports the typed calls and reaches these through the plumbing entries "filter" and "generate_batch_filtered".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_filter.h"
#include "gpsiq_filter_plan.h"

using namespace gpsiq;

namespace {

struct TapStats { long mag = 0; int max_tap = 0; };

// what both calls ask of the filter itself
int check_taps(const int16_t *taps, int ntaps, int shift, int decim, int sample_size, int out_sample_size, TapStats *st)
{
    if (int rc = check_formats(sample_size, out_sample_size)) return rc;
    if (ntaps < 1 || ntaps > kFiltMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kFiltMaxTaps);
    if (decim < 1 || decim > kFiltMaxDecim) return fail(GPSIQ_E_ARG, "decim %d outside 1..%d", decim, kFiltMaxDecim);
    if (shift < 0 || shift > kFiltMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kFiltMaxShift);
    if (!taps) return fail(GPSIQ_E_ARG, "null taps");
    st->max_tap = -32768;
    for (int k = 0; k < ntaps; ++k) {
        st->mag += taps[k] < 0 ? -(long) taps[k] : (long) taps[k];
        if (taps[k] > st->max_tap) st->max_tap = taps[k];
    }
    if (st->mag > kFiltTapSum) return fail(GPSIQ_E_RANGE, "sum |taps| %ld above %ld: the accumulator would not hold the sum", st->mag, kFiltTapSum);
    return GPSIQ_OK;
}

static_assert(kFiltAuto == 0 && kFiltForceGeneric == 1 && kFiltForceMfma == 2, "forced_kernel's values (gpsiq_stage_call.h)");

void note_plan(gpsiq_ctx *c, const FilterPlan &p, long pieces)
{
    c->filt.last[0] = p.launch ? (long) p.kernel : -1; c->filt.last[1] = (long) p.grid; c->filt.last[2] = (long) p.run; c->filt.last[3] = pieces;
}

// The coefficients of a call, page-locked, then queued for the device on s: the taps as dwords, and behind them the two digit planes
// of the matrix kernel (filter_build_planes, gpsiq_filter_plan.h).
// The caller has made sure nothing queued earlier still reads h_coef (every call ends synchronised).
int stage_coefficients(gpsiq_ctx *c, const int16_t *taps, int ntaps, int decim, const FilterPlan &p, hipStream_t s)
{
    FirSet &k = c->filt;
    int32_t *t32 = reinterpret_cast<int32_t *>(k.h_coef.get());
    for (int i = 0; i < ntaps; ++i) t32[i] = taps[i];
    size_t bytes = FirSet::kTapBytes;
    if (p.kernel == kFiltMfma) {
        filter_build_planes(taps, ntaps, decim, p.steps, reinterpret_cast<int8_t *>(k.h_coef.get() + FirSet::kTapBytes));
        bytes += (size_t) filter_mfma_plane_bytes(p.steps);
    }
    HIP_TRY(hipMemcpyAsync(k.d_coef.get(), k.h_coef.get(), bytes, hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

// the filter queued on s behind its coefficients: the counter is NOT zeroed here (the batch call adds its pieces up)
int queue_filter(gpsiq_ctx *c, const FilterPlan &p, int nsamp, int sample_size, const uint8_t *src, const uint8_t *head, int ntaps, int shift, int decim,
                 int phase, int out_sample_size, uint8_t *dst, hipStream_t s)
{
    FirSet &k = c->filt;
    if (p.kernel == kFiltMfma) {
        const FilterMfmaFn kernel = filter_mfma_kernel(out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no matrix filter kernel for %d-byte outputs", out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, (const uint8_t *) (k.d_coef.get() + FirSet::kTapBytes), ntaps,
                           shift, decim, phase, dst, p.nout, p.run, p.runs, p.steps, k.clip.d_count.get());
    } else {
        const FilterGenericFn kernel = filter_generic_kernel(sample_size, out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no filter kernel for %d-byte samples to %d-byte outputs", sample_size, out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, s, src, nsamp, head, reinterpret_cast<const int32_t *>(k.d_coef.get()), ntaps, shift,
                           decim, phase, dst, p.nout, p.run, p.runs, k.clip.d_count.get());
    }
    HIP_TRY(hipGetLastError());
    return GPSIQ_OK;
}

}  // namespace

int gpsiq_filter_impl(gpsiq_ctx_t *c, int nsamp, int sample_size, const void *src, const void *head, const int16_t *taps, int ntaps, int shift, int decim,
                      int phase, int out_sample_size, void *dst, void *hip_stream, int *nout, uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    TapStats st;
    if (int rc = check_taps(taps, ntaps, shift, decim, sample_size, out_sample_size, &st)) return rc;
    if (phase < 0 || phase >= decim) return fail(GPSIQ_E_ARG, "phase %d outside [0, decim %d)", phase, decim);
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    const FilterPlan p = plan_filter(nsamp, sample_size, ntaps, decim, phase, st.max_tap, forced_kernel("GPSIQ_FILTER_KERNEL", "mfma"));
    if (int rc = check_span(src, nsamp, sample_size, head, ntaps, dst, (uint64_t) p.nout, out_sample_size)) return rc;
    if (nout) *nout = p.nout;
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    note_plan(c, p, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no output: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    FirSet &k = c->filt;
    if (int rc = k.reserve()) return rc;
    if (int rc = stage_coefficients(c, taps, ntaps, decim, p, s)) return rc;
    return counted_call(k.clip, s, [&] {
        return queue_filter(c, p, nsamp, sample_size, static_cast<const uint8_t *>(src), static_cast<const uint8_t *>(head), ntaps, shift, decim, phase,
                            out_sample_size, static_cast<uint8_t *>(dst), s);
    }, clipped, kernel_ms);
}

// The pieces of gpsiq_stage_batch.h with the filter as the stage: a piece is rendered BEHIND a lead region of `hb` bytes whose last
// `hist` bytes are the ntaps - 1 samples before it, and the filter turns lead region and piece into d_out[pair].  The first piece's
// history is zeros, written per call.  Every piece is a whole number of blocks and nsamp a multiple of decim: the phase is 0 at every
// piece, and a piece's outputs are its blocks' rows back to back.
int gpsiq_generate_batch_filtered_impl(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size,
                                       const int16_t *taps, int ntaps, int shift, int decim, int out_sample_size, void *dst, size_t dst_block_stride,
                                       uint64_t *clipped, double *carr_phase_out)
{
    if (!c || (!ch && nblocks) || (!dst && nblocks && nsamp)) return fail(GPSIQ_E_ARG, "null argument");
    TapStats st;
    if (int rc = check_taps(taps, ntaps, shift, decim, sample_size, out_sample_size, &st)) return rc;
    if (int rc = check_batch_shape(nblocks, nchan, nsamp, fs)) return rc;
    if (nsamp % decim) return fail(GPSIQ_E_ARG, "nsamp %d is not a multiple of decim %d", nsamp, decim);
    const int nrow = nsamp / decim;                                   // outputs of a block
    const size_t blk_bytes = (size_t) 2 * (size_t) nsamp * (size_t) sample_size, row_bytes = (size_t) 2 * (size_t) nrow * (size_t) out_sample_size;
    if (dst_block_stride < row_bytes) return fail(GPSIQ_E_ARG, "block stride %zu too small", dst_block_stride);
    if (clipped) *clipped = 0;
    if (nblocks == 0) return GPSIQ_OK;                                // an empty batch leaves the carried phases alone
    const char *env = std::getenv("GPSIQ_FILTER_PIECE_BLOCKS");
    const int piece = filter_piece_blocks(nblocks, nsamp, blk_bytes, env ? std::atol(env) : 0);
    const size_t hist = (size_t) 2 * (size_t) (ntaps - 1) * (size_t) sample_size, hb = (hist + 15) & ~(size_t) 15;
    const int force = forced_kernel("GPSIQ_FILTER_KERNEL", "mfma");
    if (int rc = gpsiq_stage_batch_begin(c, "gpsiq_generate_batch_filtered", ch, hb + blk_bytes * (size_t) piece + 4, row_bytes * (size_t) piece + 4)) return rc;     // (+4: never a request of no bytes)
    FirSet &k = c->filt;
    if (int rc = k.reserve()) return rc;
    const StageBatch stage = {"filtered batch", sample_size, hb, hist, piece, k.clip.d_count.get(), k.clip.h_count.get()};
    const FilterPlan whole = plan_filter(piece * nsamp, sample_size, ntaps, decim, 0, st.max_tap, force);
    note_plan(c, whole, (nblocks + piece - 1) / piece);
    const hipStream_t ss = c->ring.stage_stream.get();
    const int rc0 = !nsamp ? GPSIQ_OK : [&]() -> int {
        // one kernel for every piece (the choice does not look at the length), so one set of coefficients, queued once
        if (int rc = stage_coefficients(c, taps, ntaps, decim, whole, ss)) return rc;
        HIP_TRY(hipMemsetAsync(k.clip.d_count.get(), 0, sizeof(unsigned long long), ss));
        if (hb) HIP_TRY(hipMemsetAsync(c->ring.d_render[0].get(), 0, hb, ss));       // the first block's history
        return GPSIQ_OK;
    }();
    double carr[GPSIQ_MAX_CHAN] = {};
    uint64_t clamped = 0;
    const int rc = gpsiq_stage_batch_run(c, stage, rc0, ch, nblocks, nchan, nsamp, fs, [&](const Piece &pc, PieceCopy *cp) -> int {
        uint8_t *out = c->ring.d_out[pc.pair].get();
        const FilterPlan pl = plan_filter(pc.nb * nsamp, sample_size, ntaps, decim, 0, st.max_tap, force);
        if (int rq = queue_filter(c, pl, pc.nb * nsamp, sample_size, pc.span, hist ? pc.span - hist : nullptr, ntaps, shift, decim, 0, out_sample_size, out, ss)) return rq;
        *cp = {out, row_bytes, row_bytes, (size_t) pc.nb, static_cast<uint8_t *>(dst) + (size_t) pc.b0 * dst_block_stride, dst_block_stride};
        return GPSIQ_OK;
    }, carr, &clamped);
    if (rc != GPSIQ_OK) return rc;
    if (clipped) *clipped = clamped;
    if (carr_phase_out) std::memcpy(carr_phase_out, carr, sizeof(double) * (size_t) nchan);
    return GPSIQ_OK;
}

extern "C" int gpsiq_filter_last_plan(const gpsiq_ctx_t *c, long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->filt.last[i];
    return GPSIQ_OK;
}
