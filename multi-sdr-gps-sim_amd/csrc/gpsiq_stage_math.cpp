// gpsiq_stage_math.cpp -- the plain arithmetic that goes with the noise, the output level and the stream stages (include/gpsiq_rows.h):
// what a caller works out on the host before or after a call on the device -- a noise sigma for a C/N0, the level multiplier, the
// C/N0 estimate of the correlator's sums, the steps and the decision of a search, the gains and the bits of a follow, the output count
// and the taps of a filter, the segments, the shift and the scale of a spectrum, the steps, the gains and the continuation of a mix, the
// output count, the step and the tap table of a resampler, the gain rule and the windows of a gain control, the lines of a spectrum
// and the taps of a notch, the steering and the weights of an array with and without taps.  Host code of libgpsiq_rows.so; nothing here touches a context or the
// device (the calls themselves: gpsiq_rows_link.cpp).
#include "gpsiq_internal.h"
#include "gpsiq_filter_plan.h"
#include "gpsiq_spectrum_plan.h"
#include "gpsiq_mix_geometry.h"
#include "gpsiq_resample_plan.h"
#include "gpsiq_agc_plan.h"
#include "gpsiq_cfilter_geometry.h"
#include "gpsiq_array_geometry.h"
#include "gpsiq_stap_geometry.h"

#include <algorithm>
#include <cmath>

using namespace gpsiq;

namespace {

constexpr int kWeightRows = kStapMaxRows;                              // the largest system constrained_weights solves
static_assert(kWeightRows >= kArrMaxElem && kStapWeightSum == kArrWeightSum, "one solver and one bound serve the array and the space-time array");

// c_e = exp(j 2 pi steer_cycles[e]), or e_0 where there is no steering (power inversion, element 0 the reference)
int steering_constraint(const double *steer_cycles, int nelem, long double *cr, long double *ci)
{
    typedef long double ld;
    const ld two_pi = 6.283185307179586476925286766559L;
    for (int a = 0; a < nelem; ++a) {
        if (steer_cycles) {
            if (!std::isfinite(steer_cycles[a])) return fail(GPSIQ_E_ARG, "steering phase %d not finite", a);
            cr[a] = std::cos(two_pi * (ld) steer_cycles[a]);
            ci[a] = std::sin(two_pi * (ld) steer_cycles[a]);
        } else { cr[a] = a ? 0.0L : 1.0L; ci[a] = 0.0L; }
    }
    return GPSIQ_OK;
}

// w = rint(2^shift conj(v)), v = Rn^-1 c / (c^H Rn^-1 c), Rn = cov / nsamp + loading (trace / n) I of n rows (n <= kWeightRows, the
// caller has checked every argument): the long double Cholesky of gpsiq_array_weights and gpsiq_stap_weights, the order of every sum
// the one gpsiq_array_weights has always had.  `what` names a row in the refusals
int constrained_weights(const int64_t *cov, int n, uint64_t nsamp, const long double *cr, const long double *ci, double loading, int shift, const char *what,
                        gpsiq_ctap_t *w)
{
    typedef long double ld;
    static thread_local ld lr[kWeightRows][kWeightRows], li[kWeightRows][kWeightRows];
    ld trace = 0.0L;
    for (int a = 0; a < n; ++a) trace += (ld) cov[2 * (a * n + a)] / (ld) nsamp;
    const ld load = (ld) loading * trace / (ld) n;
    // Cholesky, from the lower triangle of cov
    for (int j = 0; j < n; ++j) {
        ld d = (ld) cov[2 * (j * n + j)] / (ld) nsamp + load;
        for (int k = 0; k < j; ++k) d -= lr[j][k] * lr[j][k] + li[j][k] * li[j][k];
        if (!(d > 0.0L) || !std::isfinite((double) d)) return fail(GPSIQ_E_ARG, "the covariance is not positive definite at %s %d (loading %g)", what, j, loading);
        const ld piv = std::sqrt(d);
        lr[j][j] = piv; li[j][j] = 0.0L;
        for (int i = j + 1; i < n; ++i) {
            ld sr = (ld) cov[2 * (i * n + j)] / (ld) nsamp, si = (ld) cov[2 * (i * n + j) + 1] / (ld) nsamp;
            for (int k = 0; k < j; ++k) {                              // - L[i][k] conj(L[j][k])
                sr -= lr[i][k] * lr[j][k] + li[i][k] * li[j][k];
                si -= li[i][k] * lr[j][k] - lr[i][k] * li[j][k];
            }
            lr[i][j] = sr / piv; li[i][j] = si / piv;
        }
    }
    ld yr[kWeightRows], yi[kWeightRows], zr[kWeightRows], zi[kWeightRows], denom = 0.0L;
    for (int i = 0; i < n; ++i) {                                      // L y = c
        ld sr = cr[i], si = ci[i];
        for (int k = 0; k < i; ++k) { sr -= lr[i][k] * yr[k] - li[i][k] * yi[k]; si -= lr[i][k] * yi[k] + li[i][k] * yr[k]; }
        yr[i] = sr / lr[i][i]; yi[i] = si / lr[i][i];
        denom += yr[i] * yr[i] + yi[i] * yi[i];
    }
    for (int i = n - 1; i >= 0; --i) {                                 // L^H z = y: (L^H)[i][k] = conj(L[k][i])
        ld sr = yr[i], si = yi[i];
        for (int k = i + 1; k < n; ++k) { sr -= lr[k][i] * zr[k] + li[k][i] * zi[k]; si -= lr[k][i] * zi[k] - li[k][i] * zr[k]; }
        zr[i] = sr / lr[i][i]; zi[i] = si / lr[i][i];
    }
    if (!(denom > 0.0L)) return fail(GPSIQ_E_ARG, "the constraint has no solution");
    const ld scale = std::ldexp(1.0L, shift);
    long q[kWeightRows][2], mag = 0;
    for (int e = 0; e < n; ++e) {
        const ld re = scale * zr[e] / denom, im = -scale * zi[e] / denom;      // conj(v_e)
        if (!(std::fabs(re) < 65536.0L) || !(std::fabs(im) < 65536.0L)) return fail(GPSIQ_E_RANGE, "weight %d leaves int16 at shift %d", e, shift);
        q[e][0] = std::lrint(re); q[e][1] = std::lrint(im);
        if (q[e][0] > 32767 || q[e][0] < -32768 || q[e][1] > 32767 || q[e][1] < -32768) return fail(GPSIQ_E_RANGE, "weight %d leaves int16 at shift %d", e, shift);
        mag += std::labs(q[e][0]) + std::labs(q[e][1]);
    }
    if (mag > kArrWeightSum) return fail(GPSIQ_E_RANGE, "sum |re| + |im| %ld above %ld at shift %d", mag, kArrWeightSum, shift);
    for (int e = 0; e < n; ++e) { w[e].re = (int16_t) q[e][0]; w[e].im = (int16_t) q[e][1]; }
    return GPSIQ_OK;
}

}  // namespace

extern "C" {

// C = (250*gain)^2 (the carrier table's amplitude), N0 = 2*sigma^2/fs (I and Q each of variance sigma^2 over fs Hz)
double gpsiq_noise_sigma_for_cn0(double cn0_dbhz, double gain, double fs)
{
    return 250.0 * std::fabs(gain) * std::sqrt(fs / (2.0 * std::pow(10.0, cn0_dbhz / 10.0)));
}

// per component: a channel of amplitude 250*gain has mean square (250*gain)^2 / 2 in I and in Q, the noise sigma^2
double gpsiq_composite_rms(const double *gain, int nchan, double sigma)
{
    double p = sigma * sigma;
    for (int c = 0; gain && c < nchan; ++c) p += (250.0 * gain[c]) * (250.0 * gain[c]) / 2.0;
    return std::sqrt(p);
}

uint32_t gpsiq_level_mult(double rms_in, double rms_out)
{
    const double m = std::rint(65536.0 * rms_out / rms_in);
    if (!(m >= 1.0)) return 1u;                            // also NaN (0/0) and a negative ratio
    return m > 16777215.0 ? 16777215u : (uint32_t) m;
}

// include/gpsiq_rows.h, "Despread": the signal is the mean of the in-phase sums, the noise per component the mean of their sample
// variance and the quadrature sums' mean square; m^2 / v = seg_len * a^2 / sigma^2 and C/N0 = a^2 * fs / (2 sigma^2)
int gpsiq_cn0_estimate(const gpsiq_despread_sum_t *sums, int count, int seg_len, double fs, double *cn0_dbhz, double *one_sigma_db)
{
    if (!cn0_dbhz || !one_sigma_db) return fail(GPSIQ_E_ARG, "null argument");
    if (seg_len < 1 || !(fs > 0.0)) return fail(GPSIQ_E_ARG, "bad seg_len %d / fs %g", seg_len, fs);
    if (count < 2) return fail(GPSIQ_E_RANGE, "C/N0 estimate needs two segments or more (have %d)", count);
    if (!sums) return fail(GPSIQ_E_ARG, "null argument");
    double m = 0.0;
    for (int k = 0; k < count; ++k) m += (double) sums[k].i;
    m /= (double) count;
    double si = 0.0, sq = 0.0;
    for (int k = 0; k < count; ++k) {
        const double d = (double) sums[k].i - m, q = (double) sums[k].q;
        si += d * d;
        sq += q * q;
    }
    const double v = (si / (double) (count - 1) + sq / (double) count) / 2.0;
    if (!(m > 0.0) || !(v > 0.0)) return fail(GPSIQ_E_RANGE, "C/N0 estimate: mean %g, noise variance %g: no signal or no noise", m, v);
    const double T = (double) seg_len / fs;
    const double cn0 = 10.0 * std::log10(m * m / (2.0 * v * T));
    *cn0_dbhz = cn0;
    *one_sigma_db = (10.0 / std::log(10.0)) * std::sqrt(1.0 / (double) count + 1.0 / ((double) count * T * std::pow(10.0, cn0 / 10.0)));
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Acquisition": the steps of a search, in gpsiq_qchan_t's units and ranges
int gpsiq_acquire_steps(double fs, double f0_hz, double df_hz, uint64_t *code_step, int64_t *carr_step0, int64_t *carr_step_inc)
{
    if (!code_step || !carr_step0 || !carr_step_inc) return fail(GPSIQ_E_ARG, "null argument");
    if (!(fs > 0.0) || !std::isfinite(fs)) return fail(GPSIQ_E_ARG, "bad fs %g", fs);
    const double cs = std::rint(1.023e6 / fs * std::ldexp(1.0, GPSIQ_CODE_FRAC_BITS));
    const double c0 = std::rint(f0_hz / fs * std::ldexp(1.0, GPSIQ_CARR_FRAC_BITS)), ci = std::rint(df_hz / fs * std::ldexp(1.0, GPSIQ_CARR_FRAC_BITS));
    const double lim = std::ldexp(1.0, GPSIQ_CARR_FRAC_BITS - 1);
    if (!(cs >= 1.0 && cs < std::ldexp(1.0, GPSIQ_CODE_FRAC_BITS + 1)))
        return fail(GPSIQ_E_RANGE, "code step %g at fs %g outside (0, 2^57)", cs, fs);
    if (!(std::fabs(c0) < lim) || !(std::fabs(ci) < lim))
        return fail(GPSIQ_E_RANGE, "carrier steps %g, %g at fs %g: |f / fs| must stay below 0.5", c0, ci, fs);
    *code_step = (uint64_t) cs;
    *carr_step0 = (int64_t) c0;
    *carr_step_inc = (int64_t) ci;
    return GPSIQ_OK;
}

// ibid.: the best cell of one satellite's grid against the largest cell away from its shift
int gpsiq_acquire_decide(const double *power, int ndopp, int nshift, int guard, int *dopp, int *shift, double *ratio)
{
    if (!power || !dopp || !shift || !ratio) return fail(GPSIQ_E_ARG, "null argument");
    if (ndopp < 1 || nshift < 1 || guard < 0) return fail(GPSIQ_E_ARG, "bad grid %d x %d / guard %d", ndopp, nshift, guard);
    int bd = 0, bs = 0;
    double best = power[0];
    for (int d = 0; d < ndopp; ++d)
        for (int s = 0; s < nshift; ++s)
            if (power[(size_t) d * (size_t) nshift + (size_t) s] > best) { best = power[(size_t) d * (size_t) nshift + (size_t) s]; bd = d; bs = s; }
    *dopp = bd; *shift = bs;
    bool have = false;
    double floor_max = 0.0;
    for (int d = 0; d < ndopp; ++d)
        for (int s = 0; s < nshift; ++s) {
            if ((int64_t) s - bs <= guard && (int64_t) bs - s <= guard) continue;
            const double v = power[(size_t) d * (size_t) nshift + (size_t) s];
            if (!have || v > floor_max) { floor_max = v; have = true; }
        }
    if (!have) return fail(GPSIQ_E_RANGE, "no cell more than %d samples from shift %d", guard, bs);
    if (!(floor_max > 0.0)) return fail(GPSIQ_E_RANGE, "the largest cell away from the peak is %g", floor_max);
    *ratio = best / floor_max;
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Follow": the loop gains of a second-order phase lock behind a first-order frequency pull-in and a carrier-aided
// first-order delay lock, in the integer units of the loop
int gpsiq_follow_gains(double fs, double fll_gain, double pll_bn_hz, double dll_bn_hz, gpsiq_follow_cfg_t *cfg)
{
    if (!cfg) return fail(GPSIQ_E_ARG, "null argument");
    for (double v : {fs, fll_gain, pll_bn_hz, dll_bn_hz})
        if (!(v > 0.0) || !std::isfinite(v)) return fail(GPSIQ_E_ARG, "fs %g, gain %g, bandwidths %g, %g: each positive and finite", fs, fll_gain, pll_bn_hz, dll_bn_hz);
    const double two_pi = 2.0 * 3.14159265358979323846, carr = std::ldexp(1.0, GPSIQ_CARR_FRAC_BITS), code = std::ldexp(1.0, GPSIQ_CODE_FRAC_BITS);
    const double n0 = fs / 1000.0, wn = pll_bn_hz / 0.53;
    const double g[4] = {std::rint(fll_gain * carr / (two_pi * n0)), std::rint(1.414 * wn / two_pi * carr / fs),
                         std::rint(wn * wn * 1e-3 / two_pi * carr / fs), std::rint(4.0 * dll_bn_hz / (2.0 * fs) * code)};
    for (double v : g)
        if (!(v >= 0.0 && v < std::ldexp(1.0, 46))) return fail(GPSIQ_E_RANGE, "gain %g at fs %g outside [0, 2^46)", v, fs);
    cfg->spacing = UINT64_C(1) << (GPSIQ_CODE_FRAC_BITS - 1);
    cfg->pull_epochs = 100;
    cfg->reserved = 0;
    cfg->kf = (int64_t) g[0]; cfg->kp = (int64_t) g[1]; cfg->ki = (int64_t) g[2]; cfg->kd = (int64_t) g[3];
    return GPSIQ_OK;
}

// ibid.: the bit edge is where 20-epoch sums of the in-phase prompt are largest; the bits are those sums' signs
int gpsiq_follow_bits(const gpsiq_follow_epoch_t *epochs, int nepochs, int skip, int *offset, int8_t *bits, int max_bits, int *nbits)
{
    if (!epochs || !offset || !nbits || (!bits && max_bits > 0)) return fail(GPSIQ_E_ARG, "null argument");
    if (skip < 0 || max_bits < 0) return fail(GPSIQ_E_ARG, "skip %d / max_bits %d", skip, max_bits);
    const int64_t n = (int64_t) nepochs - (int64_t) skip;
    if (n < 40) return fail(GPSIQ_E_RANGE, "bits need 40 epochs or more after skip (have %lld)", (long long) n);
    const gpsiq_follow_epoch_t *e = epochs + skip;
    int best = 0;
    unsigned __int128 best_sum = 0;
    for (int o = 0; o < 20; ++o) {
        unsigned __int128 total = 0;
        for (int64_t g = 0; o + 20 * (g + 1) <= n; ++g) {
            int64_t sum = 0;                                       // |ip| < 2^39: twenty of them fit
            for (int k = 0; k < 20; ++k) sum += e[o + 20 * g + k].ip;
            total += (unsigned __int128) (sum < 0 ? -sum : sum);
        }
        if (total > best_sum) { best_sum = total; best = o; }      // ascending o: the first of equals stays
    }
    const int64_t groups = (n - best) / 20;
    for (int64_t g = 0; g < groups && g < max_bits; ++g) {
        int64_t sum = 0;
        for (int k = 0; k < 20; ++k) sum += e[best + 20 * g + k].ip;
        bits[g] = (int8_t) (sum > 0 ? 1 : sum < 0 ? -1 : 0);
    }
    *offset = best;
    *nbits = (int) groups;
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Filter": the outputs of a span and the phase its continuation starts at (filter_span, gpsiq_filter_plan.h)
int gpsiq_filter_span(int nsamp, int decim, int phase, int *nout, int *next_phase)
{
    if (nsamp < 0 || decim < 1 || decim > kFiltMaxDecim || phase < 0 || phase >= decim)
        return fail(GPSIQ_E_ARG, "nsamp %d >= 0, decim %d in 1..%d, phase %d in [0, decim)", nsamp, decim, kFiltMaxDecim, phase);
    int n = 0, next = 0;
    filter_span(nsamp, decim, phase, &n, &next);
    if (nout) *nout = n;
    if (next_phase) *next_phase = next;
    return GPSIQ_OK;
}

// ibid.: a Hamming-windowed sinc low-pass as integers with a DC gain of exactly 2^shift.  Window and sinc are even about the centre
// and are evaluated at k and at ntaps - 1 - k from the same distance, so the taps are symmetric to the bit
int gpsiq_filter_design(double fs, double cutoff_hz, int ntaps, int shift, int16_t *taps)
{
    if (!taps) return fail(GPSIQ_E_ARG, "null argument");
    if (ntaps < 3 || ntaps > kFiltMaxTaps - 1 || !(ntaps & 1)) return fail(GPSIQ_E_ARG, "ntaps %d: odd, 3..%d", ntaps, kFiltMaxTaps - 1);
    if (shift < 8 || shift > 14) return fail(GPSIQ_E_ARG, "shift %d: 8..14", shift);
    if (!(fs > 0.0) || !std::isfinite(fs) || !(cutoff_hz > 0.0) || !(cutoff_hz < fs / 2.0))
        return fail(GPSIQ_E_ARG, "cutoff %g Hz outside (0, fs / 2) at fs %g", cutoff_hz, fs);
    const double pi = 3.14159265358979323846, w = 2.0 * cutoff_hz / fs;
    const int mid = (ntaps - 1) / 2;
    double h[kFiltMaxTaps], sum = 0.0;
    for (int d = 0; d <= mid; ++d) {                                   // distance from the centre
        const double x = w * (double) d, sinc = d ? std::sin(pi * x) / (pi * x) : 1.0;
        const double win = 0.54 - 0.46 * std::cos(2.0 * pi * (double) (mid - d) / (double) (ntaps - 1));
        h[mid - d] = h[mid + d] = w * sinc * win;
        sum += d ? 2.0 * h[mid + d] : h[mid];
    }
    const double scale = std::ldexp(1.0, shift) / sum;
    long total = 0, mag = 0;
    long q[kFiltMaxTaps];
    for (int k = 0; k < ntaps; ++k) { q[k] = std::lrint(h[k] * scale); total += q[k]; }
    q[mid] += (1L << shift) - total;                                   // the remainder of the rounding, to the centre tap
    for (int k = 0; k < ntaps; ++k) mag += q[k] < 0 ? -q[k] : q[k];
    if (mag > kFiltTapSum || q[mid] > 32767 || q[mid] < -32768) return fail(GPSIQ_E_RANGE, "taps outside the filter's range (sum |taps| %ld)", mag);
    for (int k = 0; k < ntaps; ++k) taps[k] = (int16_t) q[k];
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Spectrum": the segments and whole groups of a span (spectrum_span, gpsiq_spectrum_plan.h)
int gpsiq_spectrum_span(int nsamp, int nfft, int hop, int navg, int *nseg, int *ngroups)
{
    if (nsamp < 0 || !spectrum_shape_ok(nfft, hop, 0, navg))
        return fail(GPSIQ_E_ARG, "nsamp %d >= 0, nfft %d in {64, 128, 256, 512}, hop %d nfft/2 or nfft, navg %d >= 1", nsamp, nfft, hop, navg);
    int s = 0, g = 0;
    spectrum_span(nsamp, nfft, hop, navg, &s, &g);
    if (nseg) *nseg = s;
    if (ngroups) *ngroups = g;
    return GPSIQ_OK;
}

// ibid.: the smallest shift with 2 navg Ys^2 <= 2^64 - 1 (spectrum_fits, ibid.), or a negative error
int gpsiq_spectrum_min_shift(int sample_size, int nfft, int window, int navg)
{
    if ((sample_size != GPSIQ_SC08 && sample_size != GPSIQ_SC16) || !spectrum_shape_ok(nfft, nfft, window, navg))
        return fail(GPSIQ_E_ARG, "sample size %d, nfft %d in {64, 128, 256, 512}, window %d 0 or 1, navg %d >= 1", sample_size, nfft, window, navg);
    const int s = spectrum_min_shift(sample_size, nfft, window, navg);
    return s < 0 ? fail(GPSIQ_E_RANGE, "no shift up to %d holds the sum of %d segments", kSpecMaxShift, navg) : s;
}

// ibid.: 4^shift / (navg 250^2 G N fs), G = sum w^2 / N of the window as the bins apply it (1 rectangular, 6 Hann)
int gpsiq_spectrum_scale(int nfft, int window, int navg, int shift, double fs, double *scale)
{
    if (!scale) return fail(GPSIQ_E_ARG, "null argument");
    if (!spectrum_shape_ok(nfft, nfft, window, navg) || shift < 0 || shift > kSpecMaxShift || !(fs > 0.0) || !std::isfinite(fs))
        return fail(GPSIQ_E_ARG, "nfft %d, window %d, navg %d, shift %d in 0..%d, fs %g positive and finite", nfft, window, navg, shift, kSpecMaxShift, fs);
    *scale = std::ldexp(1.0, 2 * shift) / ((double) navg * 62500.0 * (window ? 6.0 : 1.0) * (double) nfft * fs);
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Mix": the terms of a continuation, `done` samples on -- a stream term's delay shrinks, and once it is used up
// its source moves forward; gates, sweeps and phases are functions of the absolute index and stay as they are
int gpsiq_mix_advance(gpsiq_mix_term_t *terms, int nterms, uint64_t done)
{
    if (!terms || nterms < 0 || nterms > kMixMaxTerms) return fail(GPSIQ_E_ARG, "null terms or nterms %d outside 0..%d", nterms, kMixMaxTerms);
    for (int k = 0; k < nterms; ++k) {
        gpsiq_mix_term_t &t = terms[k];
        if (t.kind != GPSIQ_MIX_STREAM && t.kind != GPSIQ_MIX_ROTATED) continue;
        if (t.sample_size != GPSIQ_SC08 && t.sample_size != GPSIQ_SC16) return fail(GPSIQ_E_ARG, "term %d: bad sample size %d", k, t.sample_size);
        if (done <= t.skip) { t.skip -= done; continue; }
        t.src = static_cast<const uint8_t *>(t.src) + (size_t) (done - t.skip) * 2 * (size_t) t.sample_size;
        t.skip = 0;
    }
    return GPSIQ_OK;
}

// ibid.: frequencies into units of 2^-59 cycle per sample (and per sample squared); half the sampling rate is 2^58
int gpsiq_mix_tone(double fs, double f0_hz, double f1_hz, double sweep_s, int64_t *step, int64_t *rate, uint32_t *sweep_period)
{
    if (!step || !rate || !sweep_period) return fail(GPSIQ_E_ARG, "null argument");
    if (!(fs > 0.0) || !std::isfinite(fs) || !std::isfinite(f0_hz) || !std::isfinite(f1_hz) || !std::isfinite(sweep_s) || sweep_s < 0.0)
        return fail(GPSIQ_E_ARG, "fs %g positive and finite, f0 %g and f1 %g finite, sweep %g finite and not negative", fs, f0_hz, f1_hz, sweep_s);
    const double unit = std::ldexp(1.0, 59), half = std::ldexp(1.0, 58);
    const double st = std::rint(f0_hz / fs * unit);
    if (!(std::fabs(st) < half)) return fail(GPSIQ_E_RANGE, "f0 %g Hz reaches half the sampling rate %g", f0_hz, fs);
    double period = 0.0, rt = 0.0;
    if (sweep_s != 0.0) {
        period = std::rint(sweep_s * fs);
        if (!(period >= 2.0) || !(period < 4294967296.0)) return fail(GPSIQ_E_RANGE, "a sweep of %g s is %g samples: outside [2, 2^32)", sweep_s, period);
        rt = std::rint((f1_hz - f0_hz) / fs / period * unit);
        if (!(std::fabs(rt * period) < half)) return fail(GPSIQ_E_RANGE, "a sweep over %g Hz reaches half the sampling rate %g", f1_hz - f0_hz, fs);
    }
    *step = (int64_t) st;
    *rate = (int64_t) rt;
    *sweep_period = (uint32_t) period;
    return GPSIQ_OK;
}

// ibid.: an amplitude in stream units into a term's integer gain; the table's amplitude is 250
int gpsiq_mix_gain(double amplitude, int kind, int shift, int32_t *gain)
{
    if (!gain) return fail(GPSIQ_E_ARG, "null argument");
    if ((kind != GPSIQ_MIX_STREAM && kind != GPSIQ_MIX_ROTATED && kind != GPSIQ_MIX_TONE) || shift < 0 || shift > kMixMaxShift || !std::isfinite(amplitude))
        return fail(GPSIQ_E_ARG, "kind %d, shift %d in 0..%d, amplitude %g finite", kind, shift, kMixMaxShift, amplitude);
    const double g = std::rint(std::ldexp(amplitude, shift) / (kind == GPSIQ_MIX_STREAM ? 1.0 : 250.0));
    if (!(std::fabs(g) < 2147483648.0)) return fail(GPSIQ_E_RANGE, "a gain of %g does not fit 32 bits: lower the shift", g);
    *gain = (int32_t) g;
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Resample": the outputs of a span and the position its continuation starts at (resample_span,
// gpsiq_resample_plan.h)
int gpsiq_resample_span(uint64_t nsamp, uint64_t pos0, uint64_t step, uint64_t *nout, uint64_t *next_pos)
{
    if (nsamp >= kRsMaxSpan || pos0 >= kRsMaxPos || step < kRsMinStep || step > kRsMaxStep)
        return fail(GPSIQ_E_ARG, "nsamp %llu below 2^60, pos0 %llu below 2^63, step %llu in 2^29..2^35", (unsigned long long) nsamp, (unsigned long long) pos0,
                    (unsigned long long) step);
    uint64_t n = 0, next = 0;
    resample_span(nsamp, pos0, step, &n, &next);
    if (nout) *nout = n;
    if (next_pos) *next_pos = next;
    return GPSIQ_OK;
}

// ibid.: input samples per output sample in units of 2^-32, for a receiver whose clock runs ppb parts per billion fast
int gpsiq_resample_step(double fs_in, double fs_out, double ppb, uint64_t *step)
{
    if (!step) return fail(GPSIQ_E_ARG, "null argument");
    if (!(fs_in > 0.0) || !std::isfinite(fs_in) || !(fs_out > 0.0) || !std::isfinite(fs_out) || !std::isfinite(ppb) || !(1.0 + ppb * 1e-9 > 0.0))
        return fail(GPSIQ_E_ARG, "rates %g, %g positive and finite, ppb %g finite and above -1e9", fs_in, fs_out, ppb);
    const double s = std::rint(std::ldexp(1.0, 32) * fs_in / (fs_out * (1.0 + ppb * 1e-9)));
    if (!(s >= (double) kRsMinStep && s <= (double) kRsMaxStep)) return fail(GPSIQ_E_RANGE, "%g Hz to %g Hz is a step of %g: outside 2^29..2^35", fs_in, fs_out, s);
    *step = (uint64_t) s;
    return GPSIQ_OK;
}

// ibid.: the rows of a Hamming-windowed sinc at the fractions r / nphases.  Tap k of row r sits at t = n / (2 nphases), n the integer
// 2 k nphases + 2 r - (ntaps - 1) nphases, and the prototype is evaluated from |n|: mirrored places get the same bits.  The rows above
// the middle are copied from their mirrors, so the mirror property does not hang on the order of a sum
int gpsiq_resample_design(uint64_t step, double bandwidth, int log2_phases, int ntaps, int shift, int16_t *taps)
{
    if (!taps) return fail(GPSIQ_E_ARG, "null argument");
    if (log2_phases < 0 || log2_phases > kRsMaxLog2Phases || ntaps < 2 || ntaps > kRsMaxTaps || ((1 << log2_phases) + 1) * ntaps > kRsMaxTable)
        return fail(GPSIQ_E_ARG, "log2_phases %d in 0..%d, ntaps %d in 2..%d, (nphases + 1) * ntaps at most %d", log2_phases, kRsMaxLog2Phases, ntaps, kRsMaxTaps,
                    kRsMaxTable);
    if (shift < 8 || shift > 14) return fail(GPSIQ_E_ARG, "shift %d: 8..14", shift);
    if (step < kRsMinStep || step > kRsMaxStep || !(bandwidth > 0.0) || !(bandwidth <= 1.0))
        return fail(GPSIQ_E_ARG, "step %llu in 2^29..2^35, bandwidth %g in (0, 1]", (unsigned long long) step, bandwidth);
    const double pi = 3.14159265358979323846;
    const double w = bandwidth * (step > kRsOne ? (double) kRsOne / (double) step : 1.0);           // 2 fc: the cutoff against half the input rate
    const int nph = 1 << log2_phases;
    const long edge = (long) (ntaps - 1) * nph;                                                     // |n| at the window's ends
    for (int r = 0; r <= nph; ++r) {
        int16_t *row = taps + (size_t) r * (size_t) ntaps;
        if (r > nph - r && r < nph) {                                                               // the mirror of a row already made
            const int16_t *m = taps + (size_t) (nph - r) * (size_t) ntaps;
            for (int k = 0; k + 1 < ntaps; ++k) row[k] = m[ntaps - 2 - k];
            row[ntaps - 1] = 0;
            continue;
        }
        double g[kRsMaxTaps], sum = 0.0;
        for (int k = 0; k < ntaps; ++k) {
            long n = 2L * k * nph + 2L * r - edge;
            if (n < 0) n = -n;
            const double t = (double) n / (double) (2 * nph), x = w * t;
            g[k] = n > edge ? 0.0 : (n ? std::sin(pi * x) / (pi * x) : 1.0) * (0.54 + 0.46 * std::cos(2.0 * pi * t / (double) (ntaps - 1)));
            sum += g[k];
        }
        if (!(sum > 0.0)) return fail(GPSIQ_E_RANGE, "row %d of the design sums to %g", r, sum);
        const double scale = std::ldexp(1.0, shift) / sum;
        long q[kRsMaxTaps], total = 0, mag = 0;
        int big = 0;
        for (int k = 0; k < ntaps; ++k) {
            q[k] = std::lrint(g[k] * scale);
            total += q[k];
            if (q[k] > q[big]) big = k;                                                             // the first of equals stays
        }
        q[big] += (1L << shift) - total;                                                            // the remainder of the rounding
        for (int k = 0; k < ntaps; ++k) mag += q[k] < 0 ? -q[k] : q[k];
        if (mag > kRsTapSum || q[big] > 32767) return fail(GPSIQ_E_RANGE, "row %d outside the resampler's range (sum |taps| %ld)", r, mag);
        for (int k = 0; k < ntaps; ++k) row[k] = (int16_t) q[k];
    }
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "AGC": the gain rule (agc_gain, gpsiq_agc_geometry.h -- the function the gains kernel evaluates) under the
// ranges of the configuration it reads
int gpsiq_agc_mult(const gpsiq_agc_cfg_t *cfg, uint64_t sumsq, uint64_t count, uint32_t *mult)
{
    if (!cfg || !mult) return fail(GPSIQ_E_ARG, "null argument");
    if (cfg->target_q8 < 1 || cfg->target_q8 > kAgcMaxTarget) return fail(GPSIQ_E_ARG, "target_q8 %u outside 1..2^23-1", (unsigned) cfg->target_q8);
    if (cfg->mult_min < 1 || cfg->mult_min > cfg->mult_max || cfg->mult_max > kAgcMaxMult || cfg->mult0 < cfg->mult_min || cfg->mult0 > cfg->mult_max)
        return fail(GPSIQ_E_ARG, "multipliers: 1 <= mult_min %u <= mult0 %u <= mult_max %u < 2^24", (unsigned) cfg->mult_min, (unsigned) cfg->mult0, (unsigned) cfg->mult_max);
    if (sumsq > kAgcMaxSum || count > kAgcMaxCount) return fail(GPSIQ_E_ARG, "sum %llu at most 2^53, count %llu at most 2^23", (unsigned long long) sumsq, (unsigned long long) count);
    *mult = agc_gain(sumsq, count, cfg->target_q8, cfg->mult0, cfg->mult_min, cfg->mult_max);
    return GPSIQ_OK;
}

// ibid.: the windows a span touches and the fill it leaves (agc_span, gpsiq_agc_plan.h)
int gpsiq_agc_span(uint64_t nsamp, int window, uint32_t fill, uint64_t *nwin, uint32_t *next_fill)
{
    if (window < kAgcMinWindow || window > kAgcMaxWindow || window % 64 || fill >= (uint32_t) window || nsamp >= (UINT64_C(1) << 60))
        return fail(GPSIQ_E_ARG, "window %d a multiple of 64 in %d..%d, fill %u below it, nsamp %llu below 2^60", window, kAgcMinWindow, kAgcMaxWindow, (unsigned) fill, (unsigned long long) nsamp);
    uint64_t n = 0;
    uint32_t next = 0;
    agc_span(nsamp, (uint32_t) window, fill, &n, &next);
    if (nwin) *nwin = n;
    if (next_fill) *next_fill = next;
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Complex filter and notch": the lines of one group of a spectrum.  The median leaves at least half the cells
// at or below the floor and ratio > 1, so some cell is not over: the cyclic runs are walked from behind such a cell
int gpsiq_notch_find(const uint64_t *power, int nfft, double fs, double ratio, int max_lines, double *f_hz, double *excess_db, int *nlines)
{
    if (!power || !f_hz || !excess_db || !nlines) return fail(GPSIQ_E_ARG, "null argument");
    if (nfft < kSpecMinFft || nfft > kSpecMaxFft || (nfft & (nfft - 1))) return fail(GPSIQ_E_ARG, "nfft %d: 64, 128, 256 or 512", nfft);
    if (!(ratio > 1.0) || !std::isfinite(ratio) || !(fs > 0.0) || !std::isfinite(fs)) return fail(GPSIQ_E_ARG, "ratio %g above 1, fs %g above 0", ratio, fs);
    if (max_lines < 1 || max_lines > 8) return fail(GPSIQ_E_ARG, "max_lines %d outside 1..8", max_lines);
    uint64_t sorted[kSpecMaxFft];
    std::copy(power, power + nfft, sorted);
    std::sort(sorted, sorted + nfft);
    const uint64_t floor = sorted[nfft / 2 - 1];                       // the lower of the two middle cells
    if (floor == 0) return fail(GPSIQ_E_ARG, "the median of the spectrum is 0: no floor to compare with");
    const long double limit = (long double) ratio * (long double) floor;
    const auto over = [&](int k) { return (long double) power[k] > limit; };
    struct Line { uint64_t peak; int first; double f; };
    Line lines[kSpecMaxFft / 2];
    int found = 0, start = 0;
    while (over(start)) ++start;                                       // (ends: see above)
    for (int i = 1; i <= nfft;) {
        const int k0 = (start + i) % nfft;
        if (!over(k0)) { ++i; continue; }
        long double sum = 0.0L, moment = 0.0L;
        uint64_t peak = 0;
        int len = 0;
        for (; over((k0 + len) % nfft); ++len) {                       // stops at `start` at the latest
            const uint64_t v = power[(k0 + len) % nfft];
            sum += (long double) v;
            moment += (long double) v * (long double) len;
            if (v > peak) peak = v;
        }
        long double bin = (long double) (k0 < nfft / 2 ? k0 : k0 - nfft) + moment / sum;    // unwrapped from the run's first cell on
        if (bin >= (long double) (nfft / 2)) bin -= (long double) nfft;
        lines[found++] = {peak, k0, (double) (bin * (long double) fs / (long double) nfft)};
        i += len;
    }
    std::sort(lines, lines + found, [](const Line &a, const Line &b) { return a.peak != b.peak ? a.peak > b.peak : a.first < b.first; });
    for (int l = 0; l < found && l < max_lines; ++l) {
        f_hz[l] = lines[l].f;
        excess_db[l] = (double) (10.0L * std::log10((long double) lines[l].peak / (long double) floor));
    }
    *nlines = found;
    return GPSIQ_OK;
}

// ibid.: a linear-phase notch at nlines frequencies.  g is gpsiq_filter_design's window and sinc, unrounded, at cutoff width_hz / 2 and
// sum 1; its zero-phase response G0(w) = sum g[n] cos(w (n - c)) is real, and the unrounded filter's response is
// e^(-j w c) (1 - sum_l a_l G0(w - w_l)): zero at every w_m where  sum_l a_l G0(w_m - w_l) = 1, a real symmetric system with a unit
// diagonal.  Taps at distance d either side of the centre come from the same numbers, so taps[c + d] = conj(taps[c - d]) to the bit
int gpsiq_notch_design(double fs, const double *f_hz, int nlines, double width_hz, int ntaps, int shift, gpsiq_ctap_t *taps)
{
    if (!taps || !f_hz) return fail(GPSIQ_E_ARG, "null argument");
    if (ntaps < 3 || ntaps > kFiltMaxTaps - 1 || !(ntaps & 1)) return fail(GPSIQ_E_ARG, "ntaps %d: odd, 3..%d", ntaps, kFiltMaxTaps - 1);
    if (shift < 8 || shift > 14) return fail(GPSIQ_E_ARG, "shift %d: 8..14", shift);
    if (nlines < 1 || nlines > 8) return fail(GPSIQ_E_ARG, "nlines %d outside 1..8", nlines);
    if (!(fs > 0.0) || !std::isfinite(fs) || !(width_hz > 0.0) || !(width_hz < fs)) return fail(GPSIQ_E_ARG, "width %g Hz outside (0, fs) at fs %g", width_hz, fs);
    for (int l = 0; l < nlines; ++l) {
        if (!(std::fabs(f_hz[l]) < fs / 2.0)) return fail(GPSIQ_E_ARG, "line %d at %g Hz outside (-fs / 2, fs / 2)", l, f_hz[l]);
        for (int m = 0; m < l; ++m) {
            const double d = std::fabs(f_hz[l] - f_hz[m]), cyc = d < fs - d ? d : fs - d;
            if (cyc < width_hz) return fail(GPSIQ_E_ARG, "lines %d and %d are %g Hz apart, closer than the width %g", m, l, cyc, width_hz);
        }
    }
    const double pi = 3.14159265358979323846, w = width_hz / fs;
    const int mid = (ntaps - 1) / 2;
    double g[kFiltMaxTaps / 2], sum = 0.0;                              // by the distance from the centre
    for (int d = 0; d <= mid; ++d) {
        const double x = w * (double) d, sinc = d ? std::sin(pi * x) / (pi * x) : 1.0;
        g[d] = w * sinc * (0.54 - 0.46 * std::cos(2.0 * pi * (double) (mid - d) / (double) (ntaps - 1)));
        sum += d ? 2.0 * g[d] : g[d];
    }
    for (int d = 0; d <= mid; ++d) g[d] /= sum;
    const auto g0 = [&](double omega) { double r = g[0]; for (int d = 1; d <= mid; ++d) r += 2.0 * g[d] * std::cos(omega * (double) d); return r; };
    double om[8], m[8][9];
    for (int l = 0; l < nlines; ++l) om[l] = 2.0 * pi * f_hz[l] / fs;
    for (int r = 0; r < nlines; ++r) {
        for (int l = 0; l < nlines; ++l) m[r][l] = r == l ? 1.0 : g0(om[r] - om[l]);
        m[r][nlines] = 1.0;
    }
    for (int col = 0; col < nlines; ++col) {                           // Gauss-Jordan with partial pivoting
        int piv = col;
        for (int r = col + 1; r < nlines; ++r) if (std::fabs(m[r][col]) > std::fabs(m[piv][col])) piv = r;
        if (!(std::fabs(m[piv][col]) > 1e-9)) return fail(GPSIQ_E_ARG, "the lines' system is singular");
        for (int k = 0; k <= nlines; ++k) std::swap(m[col][k], m[piv][k]);
        for (int r = 0; r < nlines; ++r) {
            if (r == col) continue;
            const double f = m[r][col] / m[col][col];
            for (int k = col; k <= nlines; ++k) m[r][k] -= f * m[col][k];
        }
    }
    double a[8];
    for (int l = 0; l < nlines; ++l) a[l] = m[l][nlines] / m[l][l];
    const double scale = std::ldexp(1.0, shift);
    long mag = 0;
    long q[kFiltMaxTaps / 2][2];
    for (int d = 0; d <= mid; ++d) {
        double re = d ? 0.0 : 1.0, im = 0.0;
        for (int l = 0; l < nlines; ++l) { re -= a[l] * g[d] * std::cos(om[l] * (double) d); im -= a[l] * g[d] * std::sin(om[l] * (double) d); }
        q[d][0] = std::lrint(scale * re);
        q[d][1] = d ? std::lrint(scale * im) : 0;
        if (q[d][0] > 32767 || q[d][0] < -32767 || q[d][1] > 32767 || q[d][1] < -32767) return fail(GPSIQ_E_RANGE, "a tap leaves int16 at shift %d", shift);
        mag += (d ? 2 : 1) * (std::labs(q[d][0]) + std::labs(q[d][1]));
    }
    if (mag > kCfiltTapSum) return fail(GPSIQ_E_RANGE, "sum |re| + |im| %ld above %ld at shift %d", mag, kCfiltTapSum, shift);
    for (int d = 0; d <= mid; ++d) {
        taps[mid + d].re = taps[mid - d].re = (int16_t) q[d][0];
        taps[mid + d].im = (int16_t) q[d][1];
        taps[mid - d].im = (int16_t) -q[d][1];
    }
    return GPSIQ_OK;
}

// include/gpsiq_rows.h, "Array": the phase advance, in cycles in [0, 1), of a plane wave from (az, el) at every element
int gpsiq_array_steer(const double *pos, int nelem, double az_rad, double el_rad, double *phase_cycles)
{
    if (!pos || !phase_cycles) return fail(GPSIQ_E_ARG, "null argument");
    if (nelem < 1 || nelem > kArrMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kArrMaxElem);
    if (!std::isfinite(az_rad) || !std::isfinite(el_rad)) return fail(GPSIQ_E_ARG, "direction (%g, %g) not finite", az_rad, el_rad);
    const double u[3] = {std::cos(el_rad) * std::sin(az_rad), std::cos(el_rad) * std::cos(az_rad), std::sin(el_rad)};
    for (int e = 0; e < nelem; ++e) {
        const double d = pos[3 * e] * u[0] + pos[3 * e + 1] * u[1] + pos[3 * e + 2] * u[2];
        if (!std::isfinite(d)) return fail(GPSIQ_E_ARG, "element %d: position not finite", e);
        double f = d - std::floor(d);
        if (!(f < 1.0)) f = 0.0;                                       // (a tiny negative d rounds up to 1)
        phase_cycles[e] = f;
    }
    return GPSIQ_OK;
}

// ibid.: v = Rn^-1 c / (c^H Rn^-1 c) with Rn = cov / nsamp + loading (trace / nelem) I, through the Cholesky factor Rn = L L^H in
// long double (L lower triangular with a real positive diagonal: a pivot that is not positive says Rn is not positive definite):
// L y = c forwards, L^H z = y backwards, z = Rn^-1 c, and c^H z = |y|^2 is real.  w_e = rint(2^shift conj(v_e)).
// (constrained_weights below: the arithmetic, shared with gpsiq_stap_weights, where the rows are elements times taps)
int gpsiq_array_weights(const int64_t *cov, int nelem, uint64_t nsamp, const double *steer_cycles, double loading, int shift, gpsiq_ctap_t *w)
{
    if (!cov || !w) return fail(GPSIQ_E_ARG, "null argument");
    if (nelem < 1 || nelem > kArrMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kArrMaxElem);
    if (nsamp == 0) return fail(GPSIQ_E_ARG, "a covariance of no samples");
    if (!(loading >= 0.0) || !std::isfinite(loading)) return fail(GPSIQ_E_ARG, "loading %g: finite and not negative", loading);
    if (shift < 0 || shift > kArrMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kArrMaxShift);
    long double cr[kArrMaxElem], ci[kArrMaxElem];
    if (int rc = steering_constraint(steer_cycles, nelem, cr, ci)) return rc;
    return constrained_weights(cov, nelem, nsamp, cr, ci, loading, shift, "element", w);
}

// include/gpsiq_rows.h, "Space-time array": gpsiq_array_weights over the K = nelem ntaps rows k = e ntaps + t, the constraint on the
// rows of tap ref_tap alone
int gpsiq_stap_weights(const int64_t *cov, int nelem, int ntaps, uint64_t nsamp, const double *steer_cycles, int ref_tap, double loading, int shift,
                       gpsiq_ctap_t *w)
{
    if (!cov || !w) return fail(GPSIQ_E_ARG, "null argument");
    if (nelem < 1 || nelem > kStapMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kStapMaxElem);
    if (ntaps < 1 || ntaps > kStapMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kStapMaxTaps);
    if (nelem * ntaps > kStapMaxRows) return fail(GPSIQ_E_ARG, "nelem %d * ntaps %d above %d rows", nelem, ntaps, kStapMaxRows);
    if (ref_tap < 0 || ref_tap >= ntaps) return fail(GPSIQ_E_ARG, "ref_tap %d outside 0..%d", ref_tap, ntaps - 1);
    if (nsamp == 0) return fail(GPSIQ_E_ARG, "a covariance of no samples");
    if (!(loading >= 0.0) || !std::isfinite(loading)) return fail(GPSIQ_E_ARG, "loading %g: finite and not negative", loading);
    if (shift < 0 || shift > kStapMaxShift) return fail(GPSIQ_E_ARG, "shift %d outside 0..%d", shift, kStapMaxShift);
    long double er[kStapMaxElem], ei[kStapMaxElem], cr[kStapMaxRows], ci[kStapMaxRows];
    if (int rc = steering_constraint(steer_cycles, nelem, er, ei)) return rc;
    for (int e = 0; e < nelem; ++e)
        for (int t = 0; t < ntaps; ++t) {
            cr[e * ntaps + t] = t == ref_tap ? er[e] : 0.0L;
            ci[e * ntaps + t] = t == ref_tap ? ei[e] : 0.0L;
        }
    return constrained_weights(cov, nelem * ntaps, nsamp, cr, ci, loading, shift, "row", w);
}

// ibid.: one gpsiq_stap_weights per beam, in order -- the same constrained_weights with every sum in its order, so beam b is that
// call's result bit for bit (the factorisation is repeated per beam: sharing it would be a second statement of the arithmetic to
// hold equal).  A refusal ends the call; constrained_weights writes a beam only once it has passed every check, so nothing is written
// for the refused beam or any after it.
int gpsiq_stap_beam_weights(const int64_t *cov, int nelem, int ntaps, uint64_t nsamp, const double *steer_cycles, int nbeams, int ref_tap, double loading,
                            int shift, gpsiq_ctap_t *w)
{
    if (!cov || !w || !steer_cycles) return fail(GPSIQ_E_ARG, "null argument");
    if (nbeams < 1 || nbeams > GPSIQ_STAP_MAX_BEAMS) return fail(GPSIQ_E_ARG, "nbeams %d outside 1..%d", nbeams, GPSIQ_STAP_MAX_BEAMS);
    if (nelem < 1 || nelem > kStapMaxElem) return fail(GPSIQ_E_ARG, "nelem %d outside 1..%d", nelem, kStapMaxElem);
    if (ntaps < 1 || ntaps > kStapMaxTaps) return fail(GPSIQ_E_ARG, "ntaps %d outside 1..%d", ntaps, kStapMaxTaps);
    for (int b = 0; b < nbeams; ++b)
        if (int rc = gpsiq_stap_weights(cov, nelem, ntaps, nsamp, steer_cycles + (size_t) b * (size_t) nelem, ref_tap, loading, shift,
                                        w + (size_t) b * (size_t) nelem * (size_t) ntaps))
            return rc;
    return GPSIQ_OK;
}

}  // extern "C"
