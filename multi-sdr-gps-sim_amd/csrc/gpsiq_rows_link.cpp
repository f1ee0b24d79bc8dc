// gpsiq_rows_link.cpp -- libgpsiq_rows.so's end of its link to libgpsiq.so.  The rows either side of the hot path (gpsiq_refresh.cpp,
// gpsiq_stage_math.cpp, gpsiq_nav.cpp, gpsiq_rinex.cpp: include/gpsiq_rows.h, gpsiq_extras.h) are host code in a library of their own, so that the
// library a maintainer binds for the sample loop exports the boundary and nothing else.  They run on four of that library's
// internals -- the worker pool, the quantiser, the exact carrier prefix, the calling thread's error text -- which libgpsiq.so hands
// out by name through its one plumbing entry (csrc/gpsiq_plumbing.h): one pool, one quantiser and one gpsiq_last_error() for both.
#include "gpsiq_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>

namespace gpsiq {

namespace {
template <class F>
F core(const char *name)
{
    void *p = gpsiq_plumbing(name);
    if (!p) { std::fprintf(stderr, "libgpsiq_rows: libgpsiq.so has no plumbing entry '%s' (libraries of two different builds?)\n", name); std::abort(); }
    return reinterpret_cast<F>(p);
}
}  // namespace

int fail(int code, const char *fmt, ...)
{
    static const auto f = core<decltype(&set_error)>("set_error");
    char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return f(code, text);
}

void parallel_for(int n, int nthreads, int grain, void (*fn)(void *ctx, int begin, int end), void *ctx)
{
    static const auto f = core<decltype(&parallel_for)>("parallel_for");
    f(n, nthreads, grain, fn, ctx);
}

int quantize_one(const gpsiq_chan_t &ch, double delt, int nsamp, const uint64_t *carry_in, gpsiq_qchan_t *q, uint64_t *carry_out)
{
    static const auto f = core<decltype(&quantize_one)>("quantize_one");
    return f(ch, delt, nsamp, carry_in, q, carry_out);
}

void chain_carrier(gpsiq_qchan_t *q, int nblocks, int nchan, int nsamp, const bool *cont0, const uint64_t *carry0, uint64_t *carry_end, int *last_prn)
{
    static const auto f = core<decltype(&chain_carrier)>("chain_carrier");
    f(q, nblocks, nchan, nsamp, cont0, carry0, carry_end, last_prn);
}

}  // namespace gpsiq

// The output level is context state, which lives in libgpsiq.so; the typed call is exported here because the boundary library
// is at its export limit (include/gpsiq_rows.h, "Output level").
extern "C" __attribute__((visibility("default"))) int gpsiq_set_level(gpsiq_ctx_t *ctx, const gpsiq_level_t *lv)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_set_level)>("set_level");
    return f(ctx, lv);
}

// The correlator runs on the context's device and resident descriptors, which live in libgpsiq.so (csrc/gpsiq_despread.cpp); exported
// here for the same reason (include/gpsiq_rows.h, "Despread").
extern "C" __attribute__((visibility("default"))) int gpsiq_despread(gpsiq_ctx_t *ctx, int block0, int nblocks, int nsamp, int sample_size,
                                                                     const void *src, size_t block_stride_bytes, void *hip_stream, int seg_len, int clip,
                                                                     gpsiq_despread_sum_t *sums, uint8_t *prn, gpsiq_block_stats_t *stats, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_despread)>("despread");
    return f(ctx, block0, nblocks, nsamp, sample_size, src, block_stride_bytes, hip_stream, seg_len, clip, sums, prn, stats, kernel_ms);
}

// The packed stream formats (include/gpsiq_rows.h, "Packed streams"): the block length is host arithmetic; packer, unpacker and the
// packed batch call run on the context's device (csrc/gpsiq_pack.cpp) and are exported here like the correlator.
extern "C" __attribute__((visibility("default"))) size_t gpsiq_packed_block_bytes(int nsamp, int bits)
{
    if (nsamp <= 0) return 0;
    return bits == GPSIQ_PK4 ? (size_t) nsamp : bits == GPSIQ_PK2 ? ((size_t) nsamp + 1) / 2 : 0;
}

extern "C" __attribute__((visibility("default"))) int gpsiq_pack(gpsiq_ctx_t *ctx, int nblocks, int nsamp, int sample_size, const void *src_dev,
                                                                 size_t src_stride, int bits, void *dst_dev, size_t dst_stride, void *hip_stream,
                                                                 uint64_t *clipped, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_pack)>("pack");
    return f(ctx, nblocks, nsamp, sample_size, src_dev, src_stride, bits, dst_dev, dst_stride, hip_stream, clipped, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_unpack(gpsiq_ctx_t *ctx, int nblocks, int nsamp, int bits, const void *src_dev,
                                                                   size_t src_stride, int sample_size, void *dst_dev, size_t dst_stride,
                                                                   void *hip_stream, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_unpack)>("unpack");
    return f(ctx, nblocks, nsamp, bits, src_dev, src_stride, sample_size, dst_dev, dst_stride, hip_stream, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_generate_batch_packed(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan,
                                                                                  int nsamp, double fs, int bits, void *dst_host,
                                                                                  size_t dst_block_stride, double *carr_phase_out)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_generate_batch_packed)>("generate_batch_packed");
    return f(ctx, ch, nblocks, nchan, nsamp, fs, bits, dst_host, dst_block_stride, carr_phase_out);
}

// The acquisition search runs on the context's device (csrc/gpsiq_acquire.cpp) and is exported here like the correlator (include/gpsiq_rows.h,
// "Acquisition"); its two helpers, plain arithmetic, are in gpsiq_stage_math.cpp beside gpsiq_cn0_estimate.
extern "C" __attribute__((visibility("default"))) int gpsiq_acquire(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                                                                    const uint8_t *prn, int nprn, uint64_t code_step, int64_t carr_step0,
                                                                    int64_t carr_step_inc, int ndopp, int nshift, int ncoh, int nnoncoh, int hop,
                                                                    gpsiq_acquire_peak_t *peaks, double *power, gpsiq_despread_sum_t *corr, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_acquire)>("acquire");
    return f(ctx, nsamp, sample_size, src, hip_stream, prn, nprn, code_step, carr_step0, carr_step_inc, ndopp, nshift, ncoh, nnoncoh, hop, peaks, power, corr,
             kernel_ms);
}

// The follower runs on the context's device (csrc/gpsiq_follow.cpp) and is exported here like the search (include/gpsiq_rows.h, "Follow");
// gpsiq_follow_gains and gpsiq_follow_bits, plain arithmetic, are in gpsiq_stage_math.cpp beside gpsiq_acquire_decide.
extern "C" __attribute__((visibility("default"))) int gpsiq_follow(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                                                                   const gpsiq_follow_cfg_t *cfg, gpsiq_follow_state_t *state, int nprn,
                                                                   gpsiq_follow_epoch_t *epochs, int max_epochs, int *nepochs, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_follow)>("follow");
    return f(ctx, nsamp, sample_size, src, hip_stream, cfg, state, nprn, epochs, max_epochs, nepochs, kernel_ms);
}

// The filter runs on the context's device (csrc/gpsiq_filter.cpp) and is exported here like the packer (include/gpsiq_rows.h, "Filter");
// gpsiq_filter_span and gpsiq_filter_design, plain arithmetic, are in gpsiq_stage_math.cpp beside gpsiq_follow_gains.
extern "C" __attribute__((visibility("default"))) int gpsiq_filter(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head,
                                                                   const int16_t *taps, int ntaps, int shift, int decim, int phase, int out_sample_size,
                                                                   void *dst, void *hip_stream, int *nout, uint64_t *clipped, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_filter)>("filter");
    return f(ctx, nsamp, sample_size, src, head, taps, ntaps, shift, decim, phase, out_sample_size, dst, hip_stream, nout, clipped, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_generate_batch_filtered(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan,
                                                                                    int nsamp, double fs, int sample_size, const int16_t *taps, int ntaps,
                                                                                    int shift, int decim, int out_sample_size, void *dst_host,
                                                                                    size_t dst_block_stride, uint64_t *clipped, double *carr_phase_out)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_generate_batch_filtered)>("generate_batch_filtered");
    return f(ctx, ch, nblocks, nchan, nsamp, fs, sample_size, taps, ntaps, shift, decim, out_sample_size, dst_host, dst_block_stride, clipped, carr_phase_out);
}

// The spectrum runs on the context's device (csrc/gpsiq_spectrum.cpp) and is exported here like the filter (include/gpsiq_rows.h,
// "Spectrum"); gpsiq_spectrum_span, gpsiq_spectrum_min_shift and gpsiq_spectrum_scale, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_spectrum(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, void *hip_stream,
                                                                     int nfft, int hop, int window, int navg, int shift, uint64_t *power, int *ngroups,
                                                                     float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_spectrum)>("spectrum");
    return f(ctx, nsamp, sample_size, src, hip_stream, nfft, hop, window, navg, shift, power, ngroups, kernel_ms);
}

// The mixer runs on the context's device (csrc/gpsiq_mix.cpp) and is exported here like the filter (include/gpsiq_rows.h, "Mix");
// gpsiq_mix_advance, gpsiq_mix_tone and gpsiq_mix_gain, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_mix(gpsiq_ctx_t *ctx, int nsamp, uint64_t m0, const gpsiq_mix_term_t *terms, int nterms,
                                                                int shift, int qmax, int out_sample_size, void *dst, void *hip_stream, uint64_t *clipped,
                                                                float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_mix)>("mix");
    return f(ctx, nsamp, m0, terms, nterms, shift, qmax, out_sample_size, dst, hip_stream, clipped, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_generate_batch_mixed(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp,
                                                                                 double fs, int sample_size, int32_t base_gain,
                                                                                 const gpsiq_mix_term_t *tones, int ntones, uint64_t m0, int shift,
                                                                                 int qmax, void *dst_host, size_t dst_block_stride, uint64_t *clipped,
                                                                                 double *carr_phase_out)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_generate_batch_mixed)>("generate_batch_mixed");
    return f(ctx, ch, nblocks, nchan, nsamp, fs, sample_size, base_gain, tones, ntones, m0, shift, qmax, dst_host, dst_block_stride, clipped, carr_phase_out);
}

// The resampler runs on the context's device (csrc/gpsiq_resample.cpp) and is exported here like the filter (include/gpsiq_rows.h,
// "Resample"); gpsiq_resample_span, gpsiq_resample_step and gpsiq_resample_design, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_resample(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head,
                                                                     const int16_t *taps, int log2_phases, int ntaps, int shift, int interp, uint64_t step,
                                                                     uint64_t pos0, int out_sample_size, void *dst, void *hip_stream, uint64_t *nout,
                                                                     uint64_t *next_pos, uint64_t *clipped, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_resample)>("resample");
    return f(ctx, nsamp, sample_size, src, head, taps, log2_phases, ntaps, shift, interp, step, pos0, out_sample_size, dst, hip_stream, nout, next_pos, clipped,
             kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_generate_batch_resampled(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan,
                                                                                     int nsamp, double fs, int sample_size, const int16_t *taps,
                                                                                     int log2_phases, int ntaps, int shift, int interp, uint64_t step,
                                                                                     uint64_t pos0, int out_sample_size, void *dst_host,
                                                                                     uint64_t dst_capacity, uint64_t *nout, uint64_t *clipped,
                                                                                     double *carr_phase_out)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_generate_batch_resampled)>("generate_batch_resampled");
    return f(ctx, ch, nblocks, nchan, nsamp, fs, sample_size, taps, log2_phases, ntaps, shift, interp, step, pos0, out_sample_size, dst_host, dst_capacity, nout,
             clipped, carr_phase_out);
}

// The gain control runs on the context's device (csrc/gpsiq_agc.cpp) and is exported here like the filter (include/gpsiq_rows.h,
// "AGC"); gpsiq_agc_mult and gpsiq_agc_span, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_agc(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const gpsiq_agc_cfg_t *cfg,
                                                                gpsiq_agc_state_t *state, int out_sample_size, void *dst, void *hip_stream, uint32_t *mults,
                                                                uint64_t *clipped, uint64_t *blanked, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_agc)>("agc");
    return f(ctx, nsamp, sample_size, src, cfg, state, out_sample_size, dst, hip_stream, mults, clipped, blanked, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_generate_batch_agc(gpsiq_ctx_t *ctx, const gpsiq_chan_t *ch, int nblocks, int nchan, int nsamp,
                                                                               double fs, int sample_size, const gpsiq_agc_cfg_t *cfg,
                                                                               gpsiq_agc_state_t *state, int out_sample_size, void *dst_host,
                                                                               size_t dst_block_stride, uint64_t *clipped, uint64_t *blanked,
                                                                               double *carr_phase_out)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_generate_batch_agc)>("generate_batch_agc");
    return f(ctx, ch, nblocks, nchan, nsamp, fs, sample_size, cfg, state, out_sample_size, dst_host, dst_block_stride, clipped, blanked, carr_phase_out);
}

// The complex filter runs on the context's device (csrc/gpsiq_cfilter.cpp) and is exported here like the filter (include/gpsiq_rows.h,
// "Complex filter and notch"); gpsiq_notch_find and gpsiq_notch_design, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_cfilter(gpsiq_ctx_t *ctx, int nsamp, int sample_size, const void *src, const void *head,
                                                                    const gpsiq_ctap_t *taps, int ntaps, int shift, int decim, int phase,
                                                                    int out_sample_size, void *dst, void *hip_stream, int *nout, uint64_t *clipped,
                                                                    float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_cfilter)>("cfilter");
    return f(ctx, nsamp, sample_size, src, head, taps, ntaps, shift, decim, phase, out_sample_size, dst, hip_stream, nout, clipped, kernel_ms);
}

// The array stage runs on the context's device (csrc/gpsiq_array.cpp) and is exported here like the filter (include/gpsiq_rows.h,
// "Array"); gpsiq_array_steer and gpsiq_array_weights, plain arithmetic, are in gpsiq_stage_math.cpp.
extern "C" __attribute__((visibility("default"))) int gpsiq_array_cov(gpsiq_ctx_t *ctx, int nelem, const void *const *src, int nsamp, int sample_size,
                                                                      void *hip_stream, int64_t *cov, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_array_cov)>("array_cov");
    return f(ctx, nelem, src, nsamp, sample_size, hip_stream, cov, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_array_combine(gpsiq_ctx_t *ctx, int nelem, const void *const *src, int nsamp, int sample_size,
                                                                          const gpsiq_ctap_t *w, int shift, int out_sample_size, void *dst,
                                                                          void *hip_stream, uint64_t *clipped, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_array_combine)>("array_combine");
    return f(ctx, nelem, src, nsamp, sample_size, w, shift, out_sample_size, dst, hip_stream, clipped, kernel_ms);
}

// The space-time array stage runs on the context's device (csrc/gpsiq_stap.cpp) and is exported here like the array's (include/gpsiq_rows.h,
// "Space-time array"); gpsiq_stap_weights, plain arithmetic, is in gpsiq_stage_math.cpp beside gpsiq_array_weights.
extern "C" __attribute__((visibility("default"))) int gpsiq_stap_cov(gpsiq_ctx_t *ctx, int nelem, const void *const *src, const void *const *head, int nsamp,
                                                                     int sample_size, int ntaps, void *hip_stream, int64_t *cov, float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_stap_cov)>("stap_cov");
    return f(ctx, nelem, src, head, nsamp, sample_size, ntaps, hip_stream, cov, kernel_ms);
}

extern "C" __attribute__((visibility("default"))) int gpsiq_stap_combine(gpsiq_ctx_t *ctx, int nelem, const void *const *src, const void *const *head,
                                                                         int nsamp, int sample_size, const gpsiq_ctap_t *w, int ntaps, int shift,
                                                                         int out_sample_size, void *dst, void *hip_stream, uint64_t *clipped,
                                                                         float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_stap_combine)>("stap_combine");
    return f(ctx, nelem, src, head, nsamp, sample_size, w, ntaps, shift, out_sample_size, dst, hip_stream, clipped, kernel_ms);
}

// Several beams from one pass (csrc/gpsiq_stap_beams.cpp), exported here like the combiner; gpsiq_stap_beam_weights, plain arithmetic, is
// in gpsiq_stage_math.cpp beside gpsiq_stap_weights.
extern "C" __attribute__((visibility("default"))) int gpsiq_stap_beams(gpsiq_ctx_t *ctx, int nelem, const void *const *src, const void *const *head,
                                                                       int nsamp, int sample_size, const gpsiq_ctap_t *w, int ntaps, int nbeams, int shift,
                                                                       int out_sample_size, void *const *dst, void *hip_stream, uint64_t *clipped,
                                                                       float *kernel_ms)
{
    static const auto f = gpsiq::core<decltype(&gpsiq_stap_beams)>("stap_beams");
    return f(ctx, nelem, src, head, nsamp, sample_size, w, ntaps, nbeams, shift, out_sample_size, dst, hip_stream, clipped, kernel_ms);
}
