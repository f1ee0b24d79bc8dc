// gpsiq_mix.cpp -- host side of gpsiq_mix and gpsiq_generate_batch_mixed (include/gpsiq_rows.h, "Mix"): checks, plan (gpsiq_mix_plan.h,
// pure and pinned on the CPU), the carrier table on its way to the device, kernel look-up (gpsiq_mix_kernels.hip holds the kernels and
// the table of those that exist), launch, count, and the batch call's pieces.  libgpsiq_rows.so exports the typed calls and reaches
// these through the plumbing entries "mix" and "generate_batch_mixed".
// Host code: nothing here decides device code, so the file is not one of the device sources behind gpsiq_kernels_id().
#include <cstdlib>
#include <cstring>

#include "gpsiq_ctx.h"
#include "gpsiq_mix.h"
#include "gpsiq_mix_plan.h"
#include "gpsiq_tables.h"

using namespace gpsiq;

namespace {

static_assert(kMixAuto == 0 && kMixForceGeneric == 1 && kMixForceRows == 2, "forced_kernel's values (gpsiq_stage_call.h)");

// what both calls ask of the sum's end
int check_output(int shift, int qmax, int out_sample_size)
{
    if (out_sample_size != GPSIQ_SC08 && out_sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "bad output sample size %d", out_sample_size);
    if (shift < 0 || shift > kMixMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kMixMaxShift);
    const int most = out_sample_size == GPSIQ_SC08 ? 127 : 32767;
    if (qmax < 1 || qmax > most) return fail(GPSIQ_E_ARG, "qmax %d outside 1..%d", qmax, most);
    return GPSIQ_OK;
}

// what both calls ask of a term by itself; the term as the kernels take it
int check_term(const gpsiq_mix_term_t &t, int k, MixDevTerm *d)
{
    if (t.kind != GPSIQ_MIX_STREAM && t.kind != GPSIQ_MIX_ROTATED && t.kind != GPSIQ_MIX_TONE) return fail(GPSIQ_E_ARG, "term %d: bad kind %d", k, t.kind);
    if (t.reserved || t.reserved2) return fail(GPSIQ_E_ARG, "term %d: reserved fields not 0", k);
    if (t.kind == GPSIQ_MIX_TONE) {
        if (t.src || t.skip) return fail(GPSIQ_E_ARG, "term %d: a tone has no source and no delay", k);
    } else {
        if (t.sample_size != GPSIQ_SC08 && t.sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "term %d: bad sample size %d", k, t.sample_size);
        if (!t.src) return fail(GPSIQ_E_ARG, "term %d: null source", k);
        if ((uintptr_t) t.src & 3) return fail(GPSIQ_E_ARG, "term %d: source %p not 4-byte aligned", k, t.src);
    }
    if (t.gate_on > t.gate_period) return fail(GPSIQ_E_ARG, "term %d: gate_on %u above gate_period %u", k, t.gate_on, t.gate_period);
    if (t.gate_period ? t.gate_offset >= t.gate_period : t.gate_offset != 0)
        return fail(GPSIQ_E_ARG, "term %d: gate_offset %u outside [0, gate_period %u)", k, t.gate_offset, t.gate_period);
    if (t.sweep_period ? t.sweep_offset >= t.sweep_period : t.sweep_offset != 0)
        return fail(GPSIQ_E_ARG, "term %d: sweep_offset %u outside [0, sweep_period %u)", k, t.sweep_offset, t.sweep_period);
    d->src = static_cast<const uint8_t *>(t.src);
    d->skip = t.skip; d->phase0 = t.phase0; d->step = (uint64_t) t.step; d->rate = (uint64_t) t.rate;
    d->sweep_period = t.sweep_period; d->sweep_offset = t.sweep_offset;
    d->gate_period = t.gate_period; d->gate_on = t.gate_on; d->gate_offset = t.gate_offset;
    d->gain = t.gain; d->kind = t.kind; d->fmt = t.kind == GPSIQ_MIX_TONE ? GPSIQ_SC08 : t.sample_size;
    return GPSIQ_OK;
}

// the table on the device, queued on s on first use.  The caller has made sure nothing queued earlier still reads the page-locked
// staging (every call ends synchronised); have_table is set by the caller once the call has ended well
int stage_table(MixSet &k, hipStream_t s)
{
    if (k.have_table) return GPSIQ_OK;
    for (int i = 0; i < 512; ++i) k.h_table[i] = ((uint32_t) sin512(i + 128) & 0xffffu) | ((uint32_t) sin512(i) << 16);
    HIP_TRY(hipMemcpyAsync(k.d_table.get(), k.h_table.get(), 512 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    return GPSIQ_OK;
}

// the mixer queued on s: the terms are kernel arguments and cross with the launch; the counter is NOT zeroed here (the batch call
// adds its pieces up)
int queue_mix(gpsiq_ctx *c, const MixPlan &p, const MixDevTerms &terms, uint64_t m0, int nsamp, int shift, int qmax, int out_sample_size, uint8_t *dst,
              hipStream_t s)
{
    MixSet &k = c->mix;
    if (p.kernel == kMixRows) {
        const MixRowsFn kernel = mix_rows_kernel(out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no row mix kernel for %d-byte outputs", out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, terms, m0, nsamp, shift, qmax, dst, p.lead, p.units, (const uint32_t *) k.d_table.get(),
                           k.clip.d_count.get());
    } else {
        const MixGenericFn kernel = mix_generic_kernel(out_sample_size);
        if (!kernel) return fail(GPSIQ_E_DEVICE, "no mix kernel for %d-byte outputs", out_sample_size);
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), 0, s, terms, m0, nsamp, shift, qmax, dst, (const uint32_t *) k.d_table.get(), k.clip.d_count.get());
    }
    HIP_TRY(hipGetLastError());
    return GPSIQ_OK;
}

void note_plan(gpsiq_ctx *c, const MixPlan &p, long long pieces)
{
    c->mix.last[0] = p.launch ? p.kernel : -1; c->mix.last[1] = (long long) p.grid; c->mix.last[2] = (long long) p.units; c->mix.last[3] = pieces;
}

}  // namespace

int gpsiq_mix_impl(gpsiq_ctx_t *c, int nsamp, uint64_t m0, const gpsiq_mix_term_t *terms, int nterms, int shift, int qmax, int out_sample_size, void *dst,
                   void *hip_stream, uint64_t *clipped, float *kernel_ms)
{
    if (!c) return fail(GPSIQ_E_ARG, "null context");
    if (int rc = check_output(shift, qmax, out_sample_size)) return rc;
    if (nsamp < 0) return fail(GPSIQ_E_ARG, "negative size");
    if (!terms || nterms < 1 || nterms > kMixMaxTerms) return fail(GPSIQ_E_ARG, "nterms %d outside 1..%d, or null terms", nterms, kMixMaxTerms);
    if (!dst) return fail(GPSIQ_E_ARG, "null destination");
    if ((uintptr_t) dst & 3) return fail(GPSIQ_E_ARG, "destination %p not 4-byte aligned", dst);
    MixDevTerms dev = {};
    dev.n = nterms;
    const size_t dst_len = (size_t) 2 * (size_t) nsamp * (size_t) out_sample_size;
    for (int k = 0; k < nterms; ++k) {
        const gpsiq_mix_term_t &t = terms[k];
        if (int rc = check_term(t, k, &dev.t[k])) return rc;
        if (t.kind == GPSIQ_MIX_TONE) continue;
        if (t.src == dst && t.skip == 0 && t.sample_size == out_sample_size) continue;       // in place
        const size_t len = t.skip >= (uint64_t) nsamp ? 0 : (size_t) 2 * ((size_t) nsamp - (size_t) t.skip) * (size_t) t.sample_size;
        if (overlap(dst, dst_len, t.src, len))
            return fail(GPSIQ_E_ARG, "term %d: source [%p, +%zu) and destination [%p, +%zu) overlap and are not the in-place case", k, t.src, len, dst, dst_len);
    }
    const MixPlan p = plan_mix(nsamp, m0, out_sample_size, (uint64_t) (uintptr_t) dst, forced_kernel("GPSIQ_MIX_KERNEL", "rows"));
    if (clipped) *clipped = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    MixPlan none;
    note_plan(c, none, 0);
    if (!p.launch) return GPSIQ_OK;                                   // no sample: nothing to write
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t) hip_stream;
    MixSet &k = c->mix;
    if (int rc = k.reserve()) return rc;
    if (int rc = stage_table(k, s)) return rc;
    if (int rc = counted_call(k.clip, s, [&] { return queue_mix(c, p, dev, m0, nsamp, shift, qmax, out_sample_size, static_cast<uint8_t *>(dst), s); },
                              clipped, kernel_ms)) return rc;
    k.have_table = true;
    note_plan(c, p, 0);
    return GPSIQ_OK;
}

// The pieces of gpsiq_stage_batch.h with the mixer as the stage, IN PLACE: the stream term is the rendered piece itself, the tones
// run at the piece's absolute sample index, and the rows cross to the host from the rendered pair (no lead region, no output pair).
// Nothing crosses from piece to piece but the carrier phases: a tone's phase is a closed form of the absolute index.
int gpsiq_generate_batch_mixed_impl(gpsiq_ctx_t *c, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp, double fs, int sample_size, int32_t base_gain,
                                    const gpsiq_mix_term_t *tones, int ntones, uint64_t m0, int shift, int qmax, void *dst, size_t dst_block_stride,
                                    uint64_t *clipped, double *carr_phase_out)
{
    if (!c || (!ch && nblocks) || (!dst && nblocks && nsamp)) return fail(GPSIQ_E_ARG, "null argument");
    if (int rc = check_formats(sample_size, sample_size)) return rc;       // (in place: one format)
    if (int rc = check_output(shift, qmax, sample_size)) return rc;
    if (ntones < 0 || ntones > kMixMaxTerms - 1 || (ntones && !tones)) return fail(GPSIQ_E_ARG, "ntones %d outside 0..%d, or null tones", ntones, kMixMaxTerms - 1);
    if (int rc = check_batch_shape(nblocks, nchan, nsamp, fs)) return rc;
    MixDevTerms dev = {};
    dev.n = 1 + ntones;
    dev.t[0].gain = base_gain; dev.t[0].kind = GPSIQ_MIX_STREAM; dev.t[0].fmt = sample_size;
    for (int k = 0; k < ntones; ++k) {
        if (tones[k].kind != GPSIQ_MIX_TONE) return fail(GPSIQ_E_ARG, "tone %d: kind %d is not GPSIQ_MIX_TONE", k, tones[k].kind);
        if (int rc = check_term(tones[k], k, &dev.t[1 + k])) return rc;
    }
    const size_t blk_bytes = (size_t) 2 * (size_t) nsamp * (size_t) sample_size;
    if (dst_block_stride < blk_bytes) return fail(GPSIQ_E_ARG, "block stride %zu too small", dst_block_stride);
    if (clipped) *clipped = 0;
    if (nblocks == 0) return GPSIQ_OK;                                // an empty batch leaves the carried phases alone
    const char *env = std::getenv("GPSIQ_MIX_PIECE_BLOCKS");
    const int piece = mix_piece_blocks(nblocks, nsamp, blk_bytes, env ? std::atol(env) : 0);
    const int npieces = (nblocks + piece - 1) / piece;
    const int force = forced_kernel("GPSIQ_MIX_KERNEL", "rows");
    if (int rc = gpsiq_stage_batch_begin(c, "gpsiq_generate_batch_mixed", ch, blk_bytes * (size_t) piece + 16, 0)) return rc;       // (+16: never a request of no bytes)
    MixSet &k = c->mix;
    if (int rc = k.reserve()) return rc;
    const StageBatch stage = {"mixed batch", sample_size, 0, 0, piece, k.clip.d_count.get(), k.clip.h_count.get()};
    note_plan(c, MixPlan(), npieces);
    const hipStream_t ss = c->ring.stage_stream.get();
    const int rc0 = !nsamp ? GPSIQ_OK : [&]() -> int {
        if (int rc = stage_table(k, ss)) return rc;
        HIP_TRY(hipMemsetAsync(k.clip.d_count.get(), 0, sizeof(unsigned long long), ss));
        return GPSIQ_OK;
    }();
    double carr[GPSIQ_MAX_CHAN] = {};
    uint64_t clamped = 0;
    const int rc = gpsiq_stage_batch_run(c, stage, rc0, ch, nblocks, nchan, nsamp, fs, [&](const Piece &pc, PieceCopy *cp) -> int {
        const uint64_t m = m0 + (uint64_t) pc.b0 * (uint64_t) nsamp;
        const MixPlan pl = plan_mix(pc.nb * nsamp, m, sample_size, (uint64_t) (uintptr_t) pc.span, force);
        if (pc.p == 0) note_plan(c, pl, npieces);                     // (the plan looks at the span's address)
        dev.t[0].src = pc.span;
        if (int rq = queue_mix(c, pl, dev, m, pc.nb * nsamp, shift, qmax, sample_size, pc.span, ss)) return rq;
        *cp = {pc.span, blk_bytes, blk_bytes, (size_t) pc.nb, static_cast<uint8_t *>(dst) + (size_t) pc.b0 * dst_block_stride, dst_block_stride};
        return GPSIQ_OK;
    }, carr, &clamped);
    if (rc != GPSIQ_OK) return rc;
    if (nsamp) k.have_table = true;
    if (clipped) *clipped = clamped;
    if (carr_phase_out) std::memcpy(carr_phase_out, carr, sizeof(double) * (size_t) nchan);
    return GPSIQ_OK;
}

extern "C" int gpsiq_mix_last_plan(const gpsiq_ctx_t *c, long long out[4])
{
    if (!c || !out) return fail(GPSIQ_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) out[i] = c->mix.last[i];
    return GPSIQ_OK;
}
