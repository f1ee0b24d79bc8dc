/*
 * gpsiq_runahead.c — a whole scenario through the C-ABI, host code in C.
 *
 * What gps_thread_ep() does between reading the RINEX file and handing IQ blocks to the sink
 * (reference gps.c:2472-2933), with every step a libgpsiq entry point and the 10 Hz loop run
 * ahead of time, 30 s epoch by epoch:
 *
 *   gpsiq_rinex_read / gpsiq_rinex_select        readRinex2/3, ephemeris set for the start time
 *   allocate()  = the policy of allocateChannel() (gps.c:2164-2235) on gpsiq_sat_visibility,
 *                 gpsiq_nav_subframes, gpsiq_nav_message(init), gpsiq_track_init
 *   gpsiq_refresh_batch                          computeRange/computeCodePhase/gain, gps.c:2731-2765
 *   gpsiq_generate_batch                         the sample loop + pack, gps.c:2767-2846
 *   gpsiq_nav_message(roll), next ephemeris set,
 *   allocate()                                   the 30 s refresh, gps.c:2870-2909
 *
 *   gpsiq_runahead <rinex> <2|3> <week> <sec> <position> <nblocks> <nchan> <fs> <1|2> <out.bin> [almanac.sem]
 *                  [--cn0 dBHz] [--seed n] [--level rms] [--qmax n] [--pack 4|2] [--acquire [--follow seconds]]
 *                  [--filter cutoff_hz [--taps n] [--decim d]] [--spectrum nfft] [--tone f_hz,js_db[,f1_hz,sweep_s]]...
 *                  [--resample fs_out[,ppb]] [--agc rms_out,qmax[,window,navg] [--blank thresh,hold]]
 *
 * start time: GPS <week> <sec>, or the reference's -t form "YYYY/MM/DD,hh:mm:ss" as <week> with "-" as <sec>
 * (gps-sim.c:104; date2gps, gps.c:315-337, 2295: no leap seconds applied, as there).
 * position, one of
 *   xyz.bin        double[nblocks+1][3] ECEF metres, row 0 = start position (the one allocateChannel()
 *                  always uses, gps.c:2675, 2909), row k+1 = position of block k
 *   motion.csv     the reference's user-motion file (-m, gps.c:2253-2277, 2495-2505): "t,x,y,z" per 0.1 s,
 *                  same row meaning; a file shorter than nblocks+1 points shortens the run as the
 *                  reference's numd does
 *   lat,lon,h      a static receiver, degrees and metres (-l, gps.c:2337-2340, 2359-2363)
 * out.bin: the iqfile stream.  An optional eleventh argument names a SEM almanac file (the reference's almanac.sem,
 * almanac.c:73-184): its entries fill the almanac pages of subframes 4 and 5; without it those pages are empty, as with
 * the reference's --disable-almanac.
 * Receiver noise (optional, after the positional arguments): --cn0 <dB-Hz> puts a channel of gain 1.0 at that C/N0
 * (gpsiq_noise_sigma_for_cn0, gpsiq_set_noise), --seed <n> seeds it (default 0).  Without --cn0 the file is noiseless.
 * Output level (optional, same place): --level <rms> scales the stream so that the composite of the first block's channels and the
 * noise has that rms per component, in output steps, and saturates instead of wrapping; --qmax <n> is the clamp (default: full scale
 * of the format, 127 or 32767).  The multiplier is fixed for the run from the first block (gpsiq_composite_rms, gpsiq_level_mult,
 * gpsiq_set_level), so the file stays a function of the arguments alone.  Without --level the stream is the reference's.
 * Packed output (optional, same place): --pack 4 writes GPSIQ_PK4 (one byte per complex sample, fields -7..7), --pack 2 writes
 * GPSIQ_PK2 (two complex samples per byte, fields -1..1), the blocks back to back, through gpsiq_generate_batch_packed
 * (include/gpsiq_rows.h, "Packed streams").  It needs --level, sample size 1 and a --qmax inside the format (default: 7 or 1, the
 * format's own), so that the packer clamps nothing: the file is the levelled int8 stream in fewer bytes.  Anything else prints the
 * usage and exits with code 2.
 * Acquisition (optional, same place, no value): --acquire searches the run's FIRST block, as rendered, for every satellite 1..32 the way
 * a receiver that knows nothing would (gpsiq_acquire, include/gpsiq_rows.h, "Acquisition"): 21 Doppler bins of 500 Hz over +-5 kHz, every
 * shift of one millisecond, 4 dwells one millisecond apart, each the largest multiple of 64 samples within a millisecond; and prints one
 * line per satellite -- the best bin in Hz, its shift, and gpsiq_acquire_decide's ratio at a guard of 3 samples (" rendered gain g" behind
 * the satellites the block holds, g the descriptor's gain: with --cn0 c such a satellite is at c + 20 log10 g dB-Hz).  The block is searched where it lies: the page-locked buffer of gpsiq_host_alloc is device-accessible.
 * Not with --pack (the search reads int8 / int16 elements); it needs 64 samples or more in a millisecond and five milliseconds in a block.
 * Following (optional, with --acquire): --follow <seconds> then follows every satellite the search lists -- a ratio above FOLLOW_LISTED --
 * through the first <seconds> of the stream (gpsiq_follow, include/gpsiq_rows.h, "Follow") with gpsiq_follow_gains(fs, 0.25, 18, 5), the
 * gains for strong signals.  The follower's pull-in reaches 250 Hz (beyond it lies a false lock 500 Hz off), so with --follow the search
 * is widened to 41 bins of 250 Hz.  One line per satellite followed: the final Doppler in Hz, the code phase in chips at the sample it
 * stopped at, the mean prompt amplitude per sample from epoch 250 on, the bits gpsiq_follow_bits reads from there, the epochs and the
 * status.  The span is followed where it lies, like the searched block; it must lie inside the run's first call to the library (the blocks
 * up to the first 30 s boundary, 100 at the most).
 * Filter (optional, same place): --filter <cutoff Hz> renders at <fs> and writes the stream low-passed and decimated, at <fs>/d in the
 * run's own sample size, through gpsiq_generate_batch_filtered (include/gpsiq_rows.h, "Filter") with the taps of
 * gpsiq_filter_design(fs, cutoff, n, 14): --taps <n> (odd, 3..511, default 65), --decim <d> (1..16, default 1; the block length must be
 * a multiple of it).  The cutoff lies in (0, fs/2).  Every call to the library starts from a history of zeros.  The elements the
 * filter's clamp changed are counted and printed.  Not with --pack, --acquire or --follow.
 * Spectrum (optional, same place): --spectrum <nfft> (64, 128, 256 or 512) analyses the run's FIRST block, as written and where it lies
 * (page-locked, so the device reads it in place), with gpsiq_spectrum (include/gpsiq_rows.h, "Spectrum"): Hann window, half overlap, every
 * segment in one group, at gpsiq_spectrum_min_shift; it writes one "bin_hz density" line per bin, from -fs/2 up, to <out.bin>.psd --
 * density in stream units squared per Hz through gpsiq_spectrum_scale, fs the rate of the written stream.  Not with --pack.
 * Tones (optional, same place, up to four times): --tone <f Hz>,<J/S dB> adds a CW jammer at baseband frequency f, --tone <f0>,<J/S>,<f1>,
 * <sweep s> one that sweeps from f0 to f1 every <sweep s> seconds, and the run is written through gpsiq_generate_batch_mixed
 * (include/gpsiq_rows.h, "Mix"): the rendered stream at gain 1 (2^8 behind a rounding shift of 8) plus the tones, at the absolute sample
 * index of the run, clamped to --qmax (or the format's largest value) and the clamped elements counted and printed.  J/S is relative to
 * a satellite of descriptor gain 1: amplitude 250, or 250 * mult / 65536 with --level (gpsiq_mix_gain has the units).  Not with --pack or
 * --filter.
 * Resample (optional, same place): --resample <fs_out>[,<ppb>] renders at <fs> and writes the stream at <fs_out>, as a receiver samples it
 * whose clock runs <ppb> parts per billion fast (default 0), in the run's own sample size, through gpsiq_generate_batch_resampled
 * (include/gpsiq_rows.h, "Resample") at the step of gpsiq_resample_step(fs, fs_out, ppb) with the table of gpsiq_resample_design(step,
 * 0.8, 7, 16, 14): 128 phases of 16 taps, interpolated between.  The ratio lies in [1/8, 8].  The output is one stream without block
 * structure; the position runs on from call to call of the library, and every call starts from a history of zeros, as with --filter.
 * The samples written and the elements the clamp changed are printed.  Not with --pack, --filter, --tone, --acquire, --follow or
 * --spectrum.
 * Gain control (optional, same place): --agc <rms_out>,<qmax>[,<window>,<navg>] writes the stream through gpsiq_generate_batch_agc
 * (include/gpsiq_rows.h, "AGC") in the run's own sample size: a gain held over windows of <window> samples (a multiple of 64, default
 * 1024) from the power of the <navg> windows before (default 16) that brings the stream to <rms_out> output steps per component, clamped
 * to +-<qmax>; the multiplier is 65536 until the first window has completed.  --blank <thresh>,<hold> (only with --agc) zeroes every
 * sample with an element above <thresh>, as stored, and the <hold> samples behind it, and keeps them out of the power.  The state runs on
 * from call to call of the library.  The elements clipped, the samples blanked and the first and the last multiplier are printed.  With
 * --cn0, --seed, --level and --spectrum; not with --pack, --filter, --tone or --resample.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpsiq_extras.h"

#define BLOCKS_PER_CALL 100    /* bounds the page-locked staging buffer */

static int die(const char *what)
{
    fprintf(stderr, "gpsiq_runahead: %s: %s\n", what, gpsiq_last_error());
    return 1;
}

/* incGpsTime(.., 0.1) applied `steps` times to a whole-millisecond time (gps.c:1105-1124) */
static double time_after(double sec, long steps) { return round(round(sec * 1000.0) + 100.0 * (double) steps) / 1000.0; }

struct host_state {
    const gpsiq_nav_alm_sv_t *alm;                   /* 32 almanac entries, or NULL (--disable-almanac) */
    int nchan, week;
    double xyz0[3];
    const gpsiq_rinex_eph_t *eph;         /* the set in use: 32 satellites */
    const gpsiq_rinex_eph_t *sets;        /* all sets [nsets][32] */
    int nsets, ieph;
    gpsiq_nav_utc_t utc;
    gpsiq_iono_t iono;
    int allocated_sat[GPSIQ_MAX_SAT];
    gpsiq_ephem_t orbit[GPSIQ_MAX_CHAN];
    gpsiq_track_t trk[GPSIQ_MAX_CHAN];
    gpsiq_nav_state_t nav[GPSIQ_MAX_CHAN];
    uint32_t sbf[GPSIQ_MAX_CHAN][GPSIQ_N_SBF_PAGE][GPSIQ_N_DWRD_SBF];
};

/* allocateChannel(), gps.c:2164-2235: visible satellites, lowest PRN first, into the first free
 * channel; satellites that have set release theirs.  Returns the number of visible satellites. */
static int allocate(struct host_state *h, double t)
{
    int nsat = 0;
    for (int sv = 0; sv < GPSIQ_MAX_SAT; ++sv) {
        const gpsiq_rinex_eph_t *e = &h->eph[sv];
        int vis = e->vflg ? gpsiq_sat_visibility(&e->orbit, h->week, t, h->xyz0, 0.0, NULL) : -1;
        if (vis == 1) {
            ++nsat;
            if (h->allocated_sat[sv] != -1) continue;
            for (int i = 0; i < h->nchan; ++i) {
                if (h->trk[i].prn != 0) continue;
                memset(&h->trk[i], 0, sizeof h->trk[i]);
                {   /* chan[i].ipage survives release and re-allocation of a slot: only generateNavMsg touches it (gps.c:2137-2139) */
                    const int32_t ipage = h->nav[i].ipage;
                    memset(&h->nav[i], 0, sizeof h->nav[i]);
                    h->nav[i].ipage = ipage;
                }
                h->trk[i].prn = sv + 1;
                h->orbit[i] = e->orbit;
                if (gpsiq_nav_subframes(&e->nav, &h->utc, h->alm, h->sbf[i]) != GPSIQ_OK) return -1;          /* gps.c:2190 */
                if (gpsiq_nav_message(h->sbf[i], h->week, t, 1, &h->nav[i]) != GPSIQ_OK) return -1;         /* gps.c:2193 */
                h->trk[i].g0_week = h->nav[i].g0_week; h->trk[i].g0_sec = h->nav[i].g0_sec;
                memcpy(h->trk[i].dwrd, h->nav[i].dwrd, sizeof h->trk[i].dwrd);
                if (gpsiq_track_init(&h->orbit[i], &h->iono, h->week, t, h->xyz0, &h->trk[i], 1) != GPSIQ_OK) return -1;   /* gps.c:2196-2214 */
                h->allocated_sat[sv] = i;
                break;
            }
        } else if (h->allocated_sat[sv] >= 0) {                                                      /* gps.c:2224-2231 */
            h->trk[h->allocated_sat[sv]].prn = 0;
            h->allocated_sat[sv] = -1;
        }
    }
    return nsat;
}

/* gps.c:2889-2906: when the first valid satellite of the next set has its time of clock less than an
 * hour ahead, that set takes over: orbits at once, subframes rebuilt (the word buffer picks them up at
 * the next refresh). */
static int refresh_ephemeris(struct host_state *h, double t)
{
    if (h->ieph + 1 >= h->nsets) return 0;
    const gpsiq_rinex_eph_t *nxt = h->sets + (size_t) (h->ieph + 1) * GPSIQ_MAX_SAT;
    for (int sv = 0; sv < GPSIQ_MAX_SAT; ++sv) {
        if (!nxt[sv].vflg) continue;
        const double dt = (double) (nxt[sv].toc_week - h->week) * 604800.0 + (nxt[sv].nav.toc_sec - t);   /* subGpsTime, gps.c:1096-1103 */
        if (dt < 3600.0) {
            h->ieph++;
            h->eph = nxt;
            for (int i = 0; i < h->nchan; ++i) {
                if (h->trk[i].prn == 0) continue;
                const gpsiq_rinex_eph_t *e = &h->eph[h->trk[i].prn - 1];
                if (gpsiq_nav_subframes(&e->nav, &h->utc, h->alm, h->sbf[i]) != GPSIQ_OK) return -1;
                h->orbit[i] = e->orbit;
            }
        }
        break;
    }
    return 0;
}

/* --spectrum: the power spectral density of one written block (page-locked, so the device reads it in place), one line per bin */
static int run_spectrum(gpsiq_ctx_t *gq, const void *block, int nsamp, int ss, double fs, int nfft, const char *out_path)
{
    static uint64_t power[512];
    char path[4096];
    int nseg = 0, ngroups = 0;
    double scale = 0.0;
    if (snprintf(path, sizeof path, "%s.psd", out_path) >= (int) sizeof path) return -1;
    if (gpsiq_spectrum_span(nsamp, nfft, nfft / 2, 1, &nseg, NULL) != GPSIQ_OK) return -1;
    if (nseg < 1) { fprintf(stderr, "gpsiq_runahead: a block of %d samples holds no segment of %d\n", nsamp, nfft); return -1; }
    const int shift = gpsiq_spectrum_min_shift(ss, nfft, GPSIQ_WINDOW_HANN, nseg);
    if (shift < 0) return -1;
    if (gpsiq_spectrum(gq, nsamp, ss, block, NULL, nfft, nfft / 2, GPSIQ_WINDOW_HANN, nseg, shift, power, &ngroups, NULL) != GPSIQ_OK || ngroups != 1) return -1;
    if (gpsiq_spectrum_scale(nfft, GPSIQ_WINDOW_HANN, nseg, shift, fs, &scale) != GPSIQ_OK) return -1;
    FILE *f = fopen(path, "w");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return -1; }
    for (int i = 0; i < nfft; ++i) {
        const int k = (i + nfft / 2) % nfft;                                   /* from -fs/2 up */
        fprintf(f, "%.3f %.9e\n", (double) (k < nfft / 2 ? k : k - nfft) * fs / (double) nfft, (double) power[k] * scale);
    }
    fclose(f);
    printf("spectrum: %d bins of %.3f Hz, %d segments, shift %d -> %s\n", nfft, fs / (double) nfft, nseg, shift, path);
    return 0;
}

/* --acquire: the blind search of one rendered block (page-locked, so the device reads it in place), one line per satellite */
#define ACQ_BINS 21
#define ACQ_BINS_FOLLOW 41      /* with --follow: bins of 250 Hz, the follower's pull-in range */
#define FOLLOW_LISTED 2.2255    /* the ratio above which a satellite counts as found (measured: tests/test_acquire_ref.py, THRESHOLD) */
#define FOLLOW_SKIP 250         /* epochs the loops are given to settle before amplitude and bits are read */
struct found { int n; uint8_t prn[GPSIQ_MAX_SAT]; int bin[GPSIQ_MAX_SAT], shift[GPSIQ_MAX_SAT]; };
static int run_acquire(gpsiq_ctx_t *gq, const void *block, int nsamp, int ss, double fs, int ms, int ncoh, const gpsiq_chan_t *desc, int nchan,
                       int bins, double df, struct found *found)
{
    uint8_t prn[GPSIQ_MAX_SAT];
    static gpsiq_acquire_peak_t peaks[GPSIQ_MAX_SAT][ACQ_BINS_FOLLOW];
    uint64_t code_step;
    int64_t step0, step_inc;
    for (int p = 0; p < GPSIQ_MAX_SAT; ++p) prn[p] = (uint8_t) (p + 1);
    if (gpsiq_acquire_steps(fs, -5000.0, df, &code_step, &step0, &step_inc) != GPSIQ_OK) return -1;
    double *power = malloc(sizeof(double) * GPSIQ_MAX_SAT * (size_t) bins * (size_t) ms);
    if (!power) return -1;
    if (gpsiq_acquire(gq, nsamp, ss, block, NULL, prn, GPSIQ_MAX_SAT, code_step, step0, step_inc, bins, ms, ncoh, 4, ms, &peaks[0][0], power, NULL,
                      NULL) != GPSIQ_OK) { free(power); return -1; }
    found->n = 0;
    for (int p = 0; p < GPSIQ_MAX_SAT; ++p) {
        int bin = 0, shift = 0, rendered = 0;
        double ratio = 0.0, gain = 0.0;
        if (gpsiq_acquire_decide(power + (size_t) p * (size_t) bins * (size_t) ms, bins, ms, 3, &bin, &shift, &ratio) != GPSIQ_OK) ratio = 0.0;
        for (int i = 0; i < nchan; ++i)
            if (desc[i].prn == p + 1) { rendered = 1; gain = desc[i].gain; }
        printf("acquire PRN %2d  %+6.0f Hz  shift %5d  ratio %.4f", p + 1, -5000.0 + df * bin, shift, ratio);
        if (rendered) printf("  rendered gain %.4f", gain);
        printf("\n");
        if (ratio > FOLLOW_LISTED) { found->prn[found->n] = (uint8_t) (p + 1); found->bin[found->n] = bin; found->shift[found->n] = shift; found->n++; }
    }
    free(power);
    return 0;
}

/* --follow: every satellite the search listed, from its peak through `span` samples at `stream` (page-locked: the device reads it in
 * place), one line per satellite */
static int run_follow(gpsiq_ctx_t *gq, const void *stream, int span, int ss, double fs, double df, const struct found *found)
{
    if (!found->n) return 0;
    uint64_t code_step;
    int64_t step0, step_inc;
    gpsiq_follow_cfg_t cfg;
    if (gpsiq_acquire_steps(fs, -5000.0, df, &code_step, &step0, &step_inc) != GPSIQ_OK) return -1;
    if (gpsiq_follow_gains(fs, 0.25, 18.0, 5.0, &cfg) != GPSIQ_OK) return -1;
    /* an epoch is a code period, about a millisecond: room for half as many again as the span has milliseconds */
    const int max_epochs = (int) ((double) span / fs * 1500.0) + 16;
    static gpsiq_follow_state_t st[GPSIQ_MAX_SAT];
    int nep[GPSIQ_MAX_SAT];
    gpsiq_follow_epoch_t *rec = malloc(sizeof *rec * (size_t) found->n * (size_t) max_epochs);
    int8_t *bits = malloc((size_t) max_epochs / 20 + 1);
    if (!rec || !bits) { free(rec); free(bits); return -1; }
    memset(st, 0, sizeof st);
    for (int k = 0; k < found->n; ++k) {                       /* include/gpsiq_rows.h, "Follow": from an acquisition peak */
        st[k].prn = found->prn[k];
        st[k].sample = (uint64_t) found->shift[k];
        st[k].code_step0 = st[k].code_step = code_step;
        st[k].carr_step = st[k].carr_int = step0 + (int64_t) found->bin[k] * step_inc;
    }
    if (gpsiq_follow(gq, span, ss, stream, NULL, &cfg, st, found->n, rec, max_epochs, nep, NULL) != GPSIQ_OK) { free(rec); free(bits); return -1; }
    for (int k = 0; k < found->n; ++k) {
        const gpsiq_follow_epoch_t *r = rec + (size_t) k * (size_t) max_epochs;
        double amp = 0.0;
        const int from = nep[k] > FOLLOW_SKIP ? FOLLOW_SKIP : 0;
        for (int e = from; e < nep[k]; ++e) amp += hypot((double) r[e].ip, (double) r[e].qp) / (double) r[e].nsamp;
        if (nep[k] > from) amp /= (double) (nep[k] - from);
        int offset = 0, nbits = 0;
        if (gpsiq_follow_bits(r, nep[k], FOLLOW_SKIP, &offset, bits, max_epochs / 20 + 1, &nbits) != GPSIQ_OK) nbits = 0;
        printf("follow PRN %2d  %+9.2f Hz  code %9.4f chips  amplitude %.2f  bits %d  epochs %d  status %d\n", (int) st[k].prn,
               (double) st[k].carr_step * fs / 576460752303423488.0, (double) st[k].chip + (double) st[k].code_frac / 72057594037927936.0, amp, nbits,
               nep[k], (int) st[k].status);
    }
    free(rec); free(bits);
    return 0;
}

/* --tone f_hz,js_db[,f1_hz,sweep_s]: the integers of gpsiq_mix_tone at fs and the J/S; nonzero for a value the flag refuses */
#define MAX_TONES 4
#define TONE_SHIFT 8
/* --resample: the designed table */
#define RESAMPLE_LOG2_PHASES 7
#define RESAMPLE_PHASES (1 << RESAMPLE_LOG2_PHASES)
#define RESAMPLE_TAPS 16
#define RESAMPLE_SHIFT 14
struct tone { int64_t step, rate; uint32_t period; double js_db; };
static int parse_tone(const char *arg, double fs, struct tone *t)
{
    double f0 = 0.0, js = 0.0, f1 = 0.0, sweep = 0.0;
    char extra;
    const int n = sscanf(arg, "%lf,%lf,%lf,%lf%c", &f0, &js, &f1, &sweep, &extra);
    if (n == 2) { f1 = f0; sweep = 0.0; }
    else if (n != 4 || !(sweep > 0.0)) return 1;
    if (n == 2 && strchr(strchr(arg, ',') + 1, ',')) return 1;                 /* f,js, and then something that is no number */
    if (!isfinite(js) || !(js >= -200.0) || !(js <= 200.0)) return 1;
    t->js_db = js;
    return gpsiq_mix_tone(fs, f0, f1, sweep, &t->step, &t->rate, &t->period) != GPSIQ_OK;
}

int main(int argc, char **argv)
{
    double cn0 = NAN;
    double level_rms = NAN;
    int qmax = 0;
    int pack = 0, pack_given = 0;
    uint64_t noise_seed = 0;
    int acquire = 0;
    double follow_s = NAN;
    int follow = 0;
    double filter_hz = NAN;
    int filter = 0, ftaps = 65, fdecim = 1, fopts = 0;
    int spectrum = 0, spec_nfft = 0;
    const char *tone_arg[MAX_TONES + 1];
    int ntone = 0;
    const char *resample_arg = NULL;
    int resample = 0;
    const char *agc_arg = NULL, *blank_arg = NULL;
    int agc = 0, blank = 0;
    for (;;) {                                                                                                   /* trailing flags */
        if (argc > 1 && strcmp(argv[argc - 1], "--acquire") == 0) { acquire = 1; argc -= 1; continue; }         /* the one without a value */
        if (!(argc > 3 && (strcmp(argv[argc - 2], "--cn0") == 0 || strcmp(argv[argc - 2], "--seed") == 0 || strcmp(argv[argc - 2], "--pack") == 0 ||
                        strcmp(argv[argc - 2], "--follow") == 0 || strcmp(argv[argc - 2], "--level") == 0 || strcmp(argv[argc - 2], "--qmax") == 0 ||
                        strcmp(argv[argc - 2], "--filter") == 0 || strcmp(argv[argc - 2], "--taps") == 0 || strcmp(argv[argc - 2], "--decim") == 0 ||
                        strcmp(argv[argc - 2], "--spectrum") == 0 || strcmp(argv[argc - 2], "--tone") == 0 || strcmp(argv[argc - 2], "--resample") == 0 ||
                        strcmp(argv[argc - 2], "--agc") == 0 || strcmp(argv[argc - 2], "--blank") == 0))) break;
        if (strcmp(argv[argc - 2], "--cn0") == 0) cn0 = atof(argv[argc - 1]);
        else if (strcmp(argv[argc - 2], "--pack") == 0) { pack = atoi(argv[argc - 1]); pack_given = 1; }
        else if (strcmp(argv[argc - 2], "--level") == 0) level_rms = atof(argv[argc - 1]);
        else if (strcmp(argv[argc - 2], "--follow") == 0) { follow_s = atof(argv[argc - 1]); follow = 1; }
        else if (strcmp(argv[argc - 2], "--qmax") == 0) qmax = atoi(argv[argc - 1]);
        else if (strcmp(argv[argc - 2], "--filter") == 0) { filter_hz = atof(argv[argc - 1]); filter = 1; }
        else if (strcmp(argv[argc - 2], "--taps") == 0) { ftaps = atoi(argv[argc - 1]); fopts = 1; }
        else if (strcmp(argv[argc - 2], "--decim") == 0) { fdecim = atoi(argv[argc - 1]); fopts = 1; }
        else if (strcmp(argv[argc - 2], "--spectrum") == 0) { spec_nfft = atoi(argv[argc - 1]); spectrum = 1; }
        else if (strcmp(argv[argc - 2], "--resample") == 0) { resample_arg = argv[argc - 1]; ++resample; }
        else if (strcmp(argv[argc - 2], "--agc") == 0) { agc_arg = argv[argc - 1]; ++agc; }
        else if (strcmp(argv[argc - 2], "--blank") == 0) { blank_arg = argv[argc - 1]; ++blank; }
        else if (strcmp(argv[argc - 2], "--tone") == 0) { if (ntone <= MAX_TONES) tone_arg[ntone] = argv[argc - 1]; ++ntone; }
        else noise_seed = strtoull(argv[argc - 1], NULL, 0);
        argc -= 2;
    }
    /* --acquire: rendered elements, a millisecond of 64 samples or more, five of them in a block */
    const int acq_ms = argc >= 9 ? (int) floor(atof(argv[8]) / 1000.0 + 0.5) : 0, acq_ncoh = acq_ms / 64 * 64;
    const int acq_bad = acquire && (pack_given || (argc >= 9 && (acq_ncoh < 64 || (int) floor(atof(argv[8]) / 10.0 + 0.5) < 4 * acq_ms + acq_ncoh)));
    /* --pack: 4 or 2, with --level, sample size 1 and a clamp inside the format */
    const int pack_qmax = pack == GPSIQ_PK4 ? 7 : 1;
    const int pack_bad = pack_given && ((pack != GPSIQ_PK4 && pack != GPSIQ_PK2) || isnan(level_rms) || qmax < 0 || qmax > pack_qmax ||
                                        (argc >= 10 && atoi(argv[9]) != 1));
    /* --follow: with --acquire, a positive time of 10 s at the most (a call renders 100 blocks) */
    const int follow_bad = follow && (!acquire || !(follow_s > 0.0) || !(follow_s <= 0.1 * BLOCKS_PER_CALL));
    /* --filter: a cutoff inside (0, fs/2), odd taps 3..511, a decimation 1..16 that divides the block length; on its own */
    const double fs_arg = argc >= 9 ? atof(argv[8]) : 0.0;
    const int filter_bad = (fopts && !filter) ||
                           (filter && (pack_given || acquire || follow || !(filter_hz > 0.0) || !(filter_hz < fs_arg / 2.0) || ftaps < 3 || ftaps > 511 ||
                                       !(ftaps & 1) || fdecim < 1 || fdecim > 16 || (int) floor(fs_arg / 10.0 + 0.5) % fdecim != 0));
    /* --spectrum: one of the four sizes, on rendered elements */
    const int spectrum_bad = spectrum && (pack_given || (spec_nfft != 64 && spec_nfft != 128 && spec_nfft != 256 && spec_nfft != 512));
    /* --tone: at most four, f,js or f0,js,f1,sweep with steps gpsiq_mix_tone accepts at this fs; not with --pack or --filter */
    struct tone tone[MAX_TONES];
    int tone_bad = ntone > MAX_TONES || (ntone && (pack_given || filter));
    for (int k = 0; k < ntone && !tone_bad; ++k) tone_bad = parse_tone(tone_arg[ntone - 1 - k], fs_arg, &tone[k]);     /* (read from the end: as given) */
    /* --resample: once, fs_out[,ppb] with a step gpsiq_resample_step accepts at this fs; on its own */
    uint64_t rs_step = 0;
    double rs_fs = 0.0, rs_ppb = 0.0;
    int resample_bad = resample > 1 || (resample && (pack_given || filter || fopts || ntone || acquire || follow || spectrum));
    if (resample == 1 && !resample_bad) {
        char extra;
        const int n = sscanf(resample_arg, "%lf,%lf%c", &rs_fs, &rs_ppb, &extra);
        resample_bad = (n != 1 && n != 2) || (n == 1 && strchr(resample_arg, ',')) || !(fs_arg > 0.0) ||
                       gpsiq_resample_step(fs_arg, rs_fs, rs_ppb, &rs_step) != GPSIQ_OK;
    }
    /* --agc: once, rms_out,qmax[,window,navg] inside the stage's ranges for this sample size; --blank thresh,hold only with it */
    gpsiq_agc_cfg_t agc_cfg = {1024, 16, 0, 65536, 1, (1u << 24) - 1, 0, 0, 0};
    double agc_rms = 0.0;
    int agc_bad = agc > 1 || blank > 1 || (blank && !agc) || (agc && (pack_given || filter || fopts || ntone || resample));
    if (agc == 1 && !agc_bad) {
        char extra;
        int q = 0, w = 1024, m = 16, t = 0, hold = 0;
        const int short_form = sscanf(agc_arg, "%lf,%d%c", &agc_rms, &q, &extra) == 2;
        const int long_form = !short_form && sscanf(agc_arg, "%lf,%d,%d,%d%c", &agc_rms, &q, &w, &m, &extra) == 4;
        const int most = argc >= 10 && atoi(argv[9]) == 1 ? 127 : 32767;
        agc_bad = (!short_form && !long_form) || !(agc_rms * 256.0 >= 1.0) || !(agc_rms * 256.0 < 8388607.5) || q < 1 || q > most || w < 64 || w > 65536 || w % 64 ||
                  m < 1 || m > 64;
        if (blank && !agc_bad) agc_bad = sscanf(blank_arg, "%d,%d%c", &t, &hold, &extra) != 2 || t < 1 || t > 32767 || hold < 0 || hold > 1024;
        agc_cfg.window = w; agc_cfg.navg = m; agc_cfg.target_q8 = (uint32_t) floor(agc_rms * 256.0 + 0.5); agc_cfg.qmax = q;
        agc_cfg.blank_thresh = t; agc_cfg.blank_hold = hold;
    }
    if ((argc != 11 && argc != 12) || pack_bad || acq_bad || follow_bad || filter_bad || spectrum_bad || tone_bad || resample_bad || agc_bad) {
        fprintf(stderr, "usage: %s rinex 2|3 week sec xyz.bin|motion.csv|lat,lon,h nblocks nchan fs 1|2 out.bin [almanac.sem] [--cn0 dBHz] [--seed n] [--level rms] [--qmax n] [--pack 4|2] [--acquire [--follow seconds]] [--filter cutoff_hz [--taps n] [--decim d]] [--spectrum nfft] [--tone f_hz,js_db[,f1_hz,sweep_s]]... [--resample fs_out[,ppb]] [--agc rms_out,qmax[,window,navg] [--blank thresh,hold]]\n"
                        "       --pack needs --level, sample size 1 and --qmax <= 7 (4 bits) or <= 1 (2 bits)\n"
                        "       --acquire searches rendered elements (not with --pack) and needs fs >= 64 kHz\n"
                        "       --follow needs --acquire and a time in (0, 10] seconds inside the blocks before the first 30 s boundary\n"
                        "       --filter needs a cutoff in (0, fs/2), odd --taps 3..511 (default 65), --decim 1..16 (default 1) dividing the block length;\n"
                        "                not with --pack, --acquire or --follow\n"
                        "       --spectrum needs 64, 128, 256 or 512; not with --pack\n"
                        "       --tone (up to four) needs f,J/S or f0,J/S,f1,sweep: frequencies inside (-fs/2, fs/2), a sweep of 2 samples or more;\n"
                        "              not with --pack or --filter\n"
                        "       --resample needs a rate between fs/8 and 8 fs and, behind a comma, a clock offset in parts per billion; once, and\n"
                        "              not with --pack, --filter, --tone, --acquire, --follow or --spectrum\n"
                        "       --agc needs an output rms in [1/256, 32768) steps, a clamp 1..127 (sample size 1) or 1..32767, and optionally a window\n"
                        "             (a multiple of 64, 64..65536; default 1024) and the windows averaged (1..64; default 16); once, and not with\n"
                        "             --pack, --filter, --tone or --resample.  --blank needs --agc, a threshold 1..32767 and a hold 0..1024\n", argv[0]);
        return 2;
    }
    if (pack && !qmax) qmax = pack_qmax;
    const int version = atoi(argv[2]), nchan = atoi(argv[7]), ss = atoi(argv[9]);
    int nblocks = atoi(argv[6]), week = atoi(argv[3]);
    double sec0 = atof(argv[4]);
    const double fs = atof(argv[8]);
    if (strchr(argv[3], '/')) {                                                /* the -t form */
        int y, mo, d, hh, mi;
        double s;
        if (sscanf(argv[3], "%d/%d/%d,%d:%d:%lf", &y, &mo, &d, &hh, &mi, &s) != 6) { fprintf(stderr, "bad start time %s\n", argv[3]); return 2; }
        gpsiq_date_to_gps(y, mo, d, hh, mi, s, &week, &sec0);                 /* gps-sim.c:104, gps.c:2295 */
    }
    const int nsamp = (int) floor(fs / 10.0 + 0.5);                           /* NUM_IQ_SAMPLES, sdr.h:26 */
    if (nblocks < 0 || nchan < 1 || nchan > GPSIQ_MAX_CHAN || (ss != 1 && ss != 2)) { fprintf(stderr, "bad arguments\n"); return 2; }

    static gpsiq_rinex_eph_t eph[GPSIQ_EPHEM_SETS][GPSIQ_MAX_SAT];
    static struct host_state h;
    const int nsets = gpsiq_rinex_read(argv[1], version, &eph[0][0], &h.utc);
    if (nsets <= 0) { fprintf(stderr, "gpsiq_runahead: cannot read %s (%d)\n", argv[1], nsets); return 1; }
    const int ieph = gpsiq_rinex_select(&eph[0][0], nsets, week, sec0);        /* gps.c:2588-2608 */
    if (ieph < 0) { fprintf(stderr, "gpsiq_runahead: no ephemeris for the start time\n"); return 1; }

    double *xyz = malloc(sizeof(double) * 3 * ((size_t) nblocks + 1));
    if (!xyz) { fprintf(stderr, "cannot allocate positions\n"); return 1; }
    const size_t plen = strlen(argv[5]);
    double llh[3];
    if (plen > 4 && strcmp(argv[5] + plen - 4, ".csv") == 0) {
        const int npoints = gpsiq_motion_read_csv(argv[5], xyz, nblocks + 1);
        if (npoints <= 0) { fprintf(stderr, "gpsiq_runahead: cannot read motion file %s\n", argv[5]); return 1; }   /* gps.c:2497-2500 */
        if (npoints - 1 < nblocks) nblocks = npoints - 1;                     /* numd points give numd - 1 blocks, gps.c:2703 */
    } else if (sscanf(argv[5], "%lf,%lf,%lf", &llh[0], &llh[1], &llh[2]) == 3) {
        llh[0] /= 57.2957795131; llh[1] /= 57.2957795131;                       /* R2D, gps.h:98 */
        gpsiq_llh_to_ecef(llh, xyz);
        for (int k = 1; k <= nblocks; ++k) memcpy(xyz + 3 * (size_t) k, xyz, sizeof(double) * 3);
    } else {
        FILE *fx = fopen(argv[5], "rb");
        if (!fx || fread(xyz, sizeof(double) * 3, (size_t) nblocks + 1, fx) != (size_t) nblocks + 1) { fprintf(stderr, "bad xyz file\n"); return 2; }
        fclose(fx);
    }

    static gpsiq_nav_alm_sv_t alm[GPSIQ_MAX_SAT];
    if (argc == 12) {
        const int nalm = gpsiq_almanac_read_sem(argv[11], alm);
        if (nalm < 0) { fprintf(stderr, "gpsiq_runahead: %s\n", gpsiq_last_error()); return 1; }
        if (nalm > 0) h.alm = alm;                                             /* no valid record: as without a file */
        for (int sv = 0; sv < GPSIQ_MAX_SAT && h.alm; ++sv) {                  /* gps.c:2640-2650: within four weeks of the start */
            if (!alm[sv].valid) continue;
            const double dt = (alm[sv].toa_sec - sec0) + (double) (alm[sv].toa_week - week) * 604800.0;
            if (dt < -4.0 * 604800.0 || dt > 4.0 * 604800.0) { fprintf(stderr, "gpsiq_runahead: invalid time of almanac\n"); return 1; }
        }
    }
    h.nchan = nchan; h.week = week; h.eph = eph[ieph]; h.sets = &eph[0][0]; h.nsets = nsets; h.ieph = ieph;
    memcpy(h.xyz0, xyz, sizeof h.xyz0);
    h.iono.enable = 1; h.iono.vflg = h.utc.vflg;
    memcpy(h.iono.alpha, h.utc.alpha, sizeof h.iono.alpha); memcpy(h.iono.beta, h.utc.beta, sizeof h.iono.beta);
    for (int sv = 0; sv < GPSIQ_MAX_SAT; ++sv) h.allocated_sat[sv] = -1;      /* gps.c:2668-2669 */
    int nsat = allocate(&h, sec0);                                             /* gps.c:2675 */
    if (nsat < 0) return die("allocate");

    gpsiq_ctx_t *gq = NULL;
    if (gpsiq_create(&gq, 0) != GPSIQ_OK) return die("create");
    {   /* GPSIQ_NCO=reference: the reference's double accumulators, as in the binding of INTEGRATION.md section 2 */
        const char *m = getenv("GPSIQ_NCO");
        if (m && strcmp(m, "reference") == 0 && gpsiq_set_nco_mode(gq, GPSIQ_NCO_REFERENCE) != GPSIQ_OK) return die("nco mode");
    }
    const double sigma = isnan(cn0) ? 0.0 : gpsiq_noise_sigma_for_cn0(cn0, 1.0, fs);
    if (!isnan(cn0)) {
        const gpsiq_noise_t nz = {noise_seed, sigma, 0};
        if (gpsiq_set_noise(gq, &nz) != GPSIQ_OK) return die("noise");
    }
    if (!isnan(level_rms) && !(level_rms > 0.0)) { fprintf(stderr, "bad --level\n"); return 2; }
    if (qmax && isnan(level_rms)) { fprintf(stderr, "--qmax needs --level\n"); return 2; }
    int level_set = isnan(level_rms);                                          /* nothing to set without --level */
    uint32_t level_mult = 0;                                                   /* the multiplier in force, 0: no level */
    gpsiq_mix_term_t tones[MAX_TONES];
    int tones_set = 0;
    uint64_t tone_clipped = 0;
    const size_t blk_bytes = pack ? gpsiq_packed_block_bytes(nsamp, pack) : (size_t) 2 * (size_t) (nsamp / fdecim) * (size_t) ss;      /* as written */
    static int16_t taps[511];
    uint64_t filter_clipped = 0;
    if (filter && gpsiq_filter_design(fs, filter_hz, ftaps, 14, taps) != GPSIQ_OK) return die("filter design");
    /* --resample: the table, and room for the most samples a call of BLOCKS_PER_CALL blocks can give */
    static int16_t rs_taps[(RESAMPLE_PHASES + 1) * RESAMPLE_TAPS];
    uint64_t rs_pos = 0, rs_room = 0, rs_written = 0, rs_clipped = 0;
    if (resample) {
        if (gpsiq_resample_design(rs_step, 0.8, RESAMPLE_LOG2_PHASES, RESAMPLE_TAPS, RESAMPLE_SHIFT, rs_taps) != GPSIQ_OK) return die("resample design");
        if (gpsiq_resample_span((uint64_t) BLOCKS_PER_CALL * (uint64_t) nsamp, 0, rs_step, &rs_room, NULL) != GPSIQ_OK) return die("resample span");
        rs_room += 1;
    }
    /* --agc: the state of the run */
    gpsiq_agc_state_t agc_state;
    memset(&agc_state, 0, sizeof agc_state);
    uint64_t agc_clipped = 0, agc_blanked = 0;
    void *buf = gpsiq_host_alloc(resample ? (size_t) rs_room * 2 * (size_t) ss : blk_bytes * BLOCKS_PER_CALL);
    gpsiq_chan_t *desc = malloc(sizeof *desc * BLOCKS_PER_CALL * (size_t) nchan);
    FILE *fo = fopen(argv[10], "wb");
    if (!buf || !desc || !fo) { fprintf(stderr, "cannot allocate / open output\n"); return 1; }

    double carr[GPSIQ_MAX_CHAN];
    int have_carr = 0, nalloc = 1;
    long done = 0;
    while (done < nblocks) {
        const double t = time_after(sec0, done);
        /* blocks up to and including the one generated at the next multiple of 30 s (igrx % 300 == 0, gps.c:2870-2878) */
        const long tenths = (long) llround(t * 10.0);
        long n = 300 - tenths % 300;
        const int roll = done + n <= nblocks;
        if (n > nblocks - done) n = nblocks - done;
        for (long b = 0; b < n; b += BLOCKS_PER_CALL) {
            const int nb = (int) (n - b < BLOCKS_PER_CALL ? n - b : BLOCKS_PER_CALL);
            if (gpsiq_refresh_batch(h.orbit, &h.iono, week, time_after(sec0, done + b), xyz + 3 * (done + b + 1), nb, nchan, 0,
                                    h.trk, desc, 0) != GPSIQ_OK) return die("refresh");
            /* carr_phase is the loop's own state (gps.c:2821): hand back what the library handed out; a
             * slot allocateChannel() just (re)initialised carries its phase_ini instead (gps.c:2209-2211) */
            for (int k = 0; k < nb; ++k)
                for (int i = 0; i < nchan; ++i)
                    desc[(size_t) k * nchan + i].carr_phase = (have_carr && k == 0 && carr[i] >= 0.0) ? carr[i] : h.trk[i].carr_phase;
            if (!level_set) {                                                  /* once, from the run's first block */
                double gain[GPSIQ_MAX_CHAN];
                int ng = 0;
                for (int i = 0; i < nchan; ++i)
                    if (desc[i].prn > 0) gain[ng++] = desc[i].gain;
                const gpsiq_level_t lv = {gpsiq_level_mult(gpsiq_composite_rms(gain, ng, sigma), level_rms), qmax ? qmax : ss == 1 ? 127 : 32767};
                if (gpsiq_set_level(gq, &lv) != GPSIQ_OK) return die("level");
                level_set = 1;
                level_mult = lv.mult;
            }
            if (pack) {
                if (gpsiq_generate_batch_packed(gq, desc, nb, nchan, nsamp, fs, pack, buf, blk_bytes, carr) != GPSIQ_OK) return die("generate packed");
            } else if (filter) {
                uint64_t clipped = 0;
                if (gpsiq_generate_batch_filtered(gq, desc, nb, nchan, nsamp, fs, ss, taps, ftaps, 14, fdecim, ss, buf, blk_bytes, &clipped, carr) != GPSIQ_OK)
                    return die("generate filtered");
                filter_clipped += clipped;
            } else if (resample) {
                uint64_t clipped = 0, nout = 0, next = 0;
                if (gpsiq_generate_batch_resampled(gq, desc, nb, nchan, nsamp, fs, ss, rs_taps, RESAMPLE_LOG2_PHASES, RESAMPLE_TAPS, RESAMPLE_SHIFT, 1, rs_step,
                                                   rs_pos, ss, buf, rs_room, &nout, &clipped, carr) != GPSIQ_OK) return die("generate resampled");
                if (gpsiq_resample_span((uint64_t) nb * (uint64_t) nsamp, rs_pos, rs_step, NULL, &next) != GPSIQ_OK) return die("resample span");
                rs_pos = next;                                                 /* the next call's first output, from its first sample */
                rs_clipped += clipped;
                rs_written += nout;
                if (fwrite(buf, (size_t) 2 * (size_t) ss, (size_t) nout, fo) != (size_t) nout) { fprintf(stderr, "short write\n"); return 1; }
                have_carr = 1;
                continue;
            } else if (agc) {
                uint64_t clipped = 0, blanked = 0;
                if (gpsiq_generate_batch_agc(gq, desc, nb, nchan, nsamp, fs, ss, &agc_cfg, &agc_state, ss, buf, blk_bytes, &clipped, &blanked, carr) != GPSIQ_OK)
                    return die("generate agc");
                agc_clipped += clipped;
                agc_blanked += blanked;
            } else if (ntone) {
                if (!tones_set) {                                              /* once: J/S against a satellite of descriptor gain 1 */
                    const double unit = level_mult ? 250.0 * (double) level_mult / 65536.0 : 250.0;
                    for (int k = 0; k < ntone; ++k) {
                        memset(&tones[k], 0, sizeof tones[k]);
                        tones[k].kind = GPSIQ_MIX_TONE;
                        tones[k].step = tone[k].step; tones[k].rate = tone[k].rate; tones[k].sweep_period = tone[k].period;
                        if (gpsiq_mix_gain(unit * pow(10.0, tone[k].js_db / 20.0), GPSIQ_MIX_TONE, TONE_SHIFT, &tones[k].gain) != GPSIQ_OK) return die("tone gain");
                    }
                    tones_set = 1;
                }
                uint64_t clipped = 0;
                if (gpsiq_generate_batch_mixed(gq, desc, nb, nchan, nsamp, fs, ss, 1 << TONE_SHIFT, tones, ntone, (uint64_t) (done + b) * (uint64_t) nsamp,
                                               TONE_SHIFT, qmax ? qmax : ss == 1 ? 127 : 32767, buf, blk_bytes, &clipped, carr) != GPSIQ_OK)
                    return die("generate mixed");
                tone_clipped += clipped;
            } else if (gpsiq_generate_batch(gq, desc, nb, nchan, nsamp, fs, ss, buf, 0, carr) != GPSIQ_OK) return die("generate");
            have_carr = 1;
            if (acquire && done == 0 && b == 0) {
                struct found found;
                if (run_acquire(gq, buf, nsamp, ss, fs, acq_ms, acq_ncoh, desc, nchan, follow ? ACQ_BINS_FOLLOW : ACQ_BINS, follow ? 250.0 : 500.0, &found) != 0)
                    return die("acquire");
                if (follow) {
                    const double span = floor(follow_s * fs + 0.5);
                    if (span > (double) nb * (double) nsamp) {
                        fprintf(stderr, "gpsiq_runahead: --follow %g s is more than the %d blocks of the run's first call\n", follow_s, nb);
                        return 2;
                    }
                    if (run_follow(gq, buf, (int) span, ss, fs, 250.0, &found) != 0) return die("follow");
                }
            }
            if (spectrum && done == 0 && b == 0 && run_spectrum(gq, buf, nsamp / fdecim, ss, fs / (double) fdecim, spec_nfft, argv[10]) != 0) return die("spectrum");
            if (fwrite(buf, blk_bytes, (size_t) nb, fo) != (size_t) nb) { fprintf(stderr, "short write\n"); return 1; }
        }
        done += n;
        if (roll) {                                                            /* gps.c:2878-2885, 2909 */
            const double tr = time_after(sec0, done);
            int prn_before[GPSIQ_MAX_CHAN];
            for (int i = 0; i < nchan; ++i) {
                prn_before[i] = h.trk[i].prn;
                if (h.trk[i].prn <= 0) continue;
                if (gpsiq_nav_message(h.sbf[i], week, tr, 0, &h.nav[i]) != GPSIQ_OK) return die("nav refresh");
                memcpy(h.trk[i].dwrd, h.nav[i].dwrd, sizeof h.trk[i].dwrd);
                h.trk[i].g0_week = h.nav[i].g0_week; h.trk[i].g0_sec = h.nav[i].g0_sec;
            }
            if (refresh_ephemeris(&h, tr) != 0) return die("ephemeris refresh");
            nsat = allocate(&h, tr);
            if (nsat < 0) return die("allocate");
            ++nalloc;
            for (int i = 0; i < nchan; ++i)          /* a re-allocated slot starts from its own phase_ini */
                if (h.trk[i].prn != prn_before[i]) carr[i] = -1.0;
        }
    }
    fclose(fo);
    printf("%d blocks, %d channels, %d allocation passes, last nsat %d, ephemeris set %d of %d\n", nblocks, nchan, nalloc, nsat, h.ieph, nsets);
    if (filter) printf("filter: cutoff %g Hz, %d taps, decimation %d, %llu elements clipped\n", filter_hz, ftaps, fdecim, (unsigned long long) filter_clipped);
    if (resample)
        printf("resample: %g Hz to %g Hz at %g ppb, step %llu / 2^32, %llu samples written, %llu elements clipped\n", fs, rs_fs, rs_ppb,
               (unsigned long long) rs_step, (unsigned long long) rs_written, (unsigned long long) rs_clipped);
    if (agc) {
        uint64_t sum = 0, cnt = 0;
        uint32_t first = 0, last = 0;
        for (uint32_t r = 0; r < agc_state.nring; ++r) { sum += agc_state.wsum[r]; cnt += agc_state.wcnt[r]; }
        if (gpsiq_agc_mult(&agc_cfg, 0, 0, &first) != GPSIQ_OK || gpsiq_agc_mult(&agc_cfg, sum, cnt, &last) != GPSIQ_OK) return die("agc multiplier");
        printf("agc: rms %g, qmax %d, window %d, navg %d, %llu elements clipped, %llu samples blanked, multiplier %u at the first window, %u at the end\n", agc_rms,
               (int) agc_cfg.qmax, (int) agc_cfg.window, (int) agc_cfg.navg, (unsigned long long) agc_clipped, (unsigned long long) agc_blanked, (unsigned) first,
               (unsigned) last);
    }
    if (ntone) printf("tones: %d, %llu elements clipped\n", ntone, (unsigned long long) tone_clipped);
    gpsiq_host_free(buf);
    gpsiq_destroy(gq);
    free(desc); free(xyz);
    return 0;
}
